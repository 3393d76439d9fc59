"""The tower GEMMs' dispatch (csrc/gemm.hip), path by path: the fp32-MFMA switch
(TTAMM_FP32_MFMA=exact), pre-split feature planes (FusedTrainStep(feature_planes=True),
ttamm_to_planes / ttamm_to_bf16) and the tile classes pick_tile_n / wgrad_class choose from the
layer widths.

  * bit-exact: towers on exact-arithmetic inputs (tests/exact_inputs.py: every product and partial
    sum exactly representable, so the result is independent of the summation order) through the
    drop-in modules under autograd; output and every gradient must equal float64 bit for bit;
  * fused step: the tile classes, the exact switch and in-batch mode against the CPU oracle at the
    project's 1e-5 (bf16: 2e-3 max, 2e-5 mean, 1e-4 losses); feature planes bit for bit against the
    default; the dropout stream across the kernels' epilogue forms;
  * single ops: the in-batch kernel under the exact switch, the plane and bf16 converters.

Environment switches are set before the engine is built and held until finish(): the workspace plan
reads them."""

from __future__ import annotations

import numpy as np
import pytest
import torch

import exact_inputs as ex
import ttamm
from helpers import LOSS_WEIGHTS, Shape, clone_model, make_problem, named_optimizer_state, rel_err, set_lr
from oracle import cpu_reference as ref
from ttamm import _lib

pytestmark = pytest.mark.gpu

TOL = 1e-5
BF16_TOL, BF16_MEAN_TOL, BF16_LOSS_TOL = 2e-3, 2e-5, 1e-4


def _set_mode(monkeypatch, *, exact: bool, generic: bool = False) -> None:
    if exact:
        monkeypatch.setenv("TTAMM_FP32_MFMA", "exact")
    else:
        monkeypatch.delenv("TTAMM_FP32_MFMA", raising=False)
    if generic:
        monkeypatch.setenv("TTAMM_GENERIC_GATE", "1")
    else:
        monkeypatch.delenv("TTAMM_GENERIC_GATE", raising=False)


def _bits_differing(a: torch.Tensor, b: torch.Tensor) -> int:
    """Number of differing bits between two fp32 tensors of one shape."""
    x = (a.contiguous().view(torch.int32) ^ b.contiguous().view(torch.int32)).cpu().numpy().view("uint8")
    return int(np.unpackbits(x).sum())


# ---------------------------------------------------------------------------------------
# B. bit-exact towers
# ---------------------------------------------------------------------------------------
MODES = {"split": (False, False, False), "exact": (True, False, False), "exact-generic": (True, True, False),
         "bf16": (False, False, True), "bf16-exact": (True, False, True)}  # (exact, generic gate, bf16 towers)
EXACT_PARAMS = [(m, c) for c in ex.CASES for m in MODES if not (c in ex.PLANE_CASES and m not in ("split", "exact"))]


@pytest.mark.parametrize("mode,case", EXACT_PARAMS, ids=[f"{m}-{c}" for m, c in EXACT_PARAMS])
def test_tower_exact_inputs_bit_exact(mode, case, monkeypatch):
    """TowerEncoder.forward in train mode and backward(gy) (ttamm_tower_train_forward / _backward)
    on the exact-arithmetic problems: the output, every feature-MLP / projection weight and bias
    gradient and the dense ID-table gradient equal the float64 evaluation bit for bit (bf16 towers:
    the float64 evaluation of bf16-rounded operands)."""
    exact, generic, bf16 = MODES[mode]
    c = ex.CASES[case]
    if generic:
        # (every exact-arithmetic case is gate-free: a sigmoid is not exact.  The generic gate under
        # the exact switch runs in test_step_exact_mfma_matches_oracle[d96-c2dims-generic])
        assert c.shape.fusion in ("sum", "concat")
        pytest.skip("TTAMM_GENERIC_GATE acts on gated fusion only; this case's fusion has no gate")
    _set_mode(monkeypatch, exact=exact, generic=generic)
    shape = Shape(**{**c.shape.__dict__, "matmul_dtype": "bf16" if bf16 else "fp32"})
    for R in c.rows:
        prob = ex.build(shape, R, c.recipe)
        want_out, want, pc = ex.reference(prob, bf16=bf16)
        assert pc.ok, str(pc)
        enc = ttamm.build_tower_encoder(prob.shape.tower_cfg(), num_embeddings=prob.shape.I, feature_dim=prob.shape.F,
                                        device="cuda")
        res = enc.load_state_dict({k: v.cuda() for k, v in prob.tower.state_dict().items()}, strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        enc.train()
        idx = prob.idx.cuda()
        out = enc({"indices": idx, "features": prob.feats.cuda()})
        out.backward(prob.gy.cuda())
        torch.cuda.synchronize()
        got_out = out.detach().cpu()
        bad = int((got_out.double() != want_out).sum())
        assert got_out.shape == want_out.shape and bad == 0, f"R={R} output: {bad} of {want_out.numel()} elements differ"
        got = {n: p.grad for n, p in enc.named_parameters()}
        assert set(got) == set(want)
        for n in sorted(want):
            g = got[n].cpu()
            assert g.dtype == torch.float32 and not g.is_sparse
            bad = int((g.double() != want[n]).sum())
            assert g.shape == want[n].shape and bad == 0, f"R={R} {n}: {bad} of {g.numel()} elements differ"
        if prob.shape.fusion == "sum":  # d(out)/d(ID row) = 1: the table gradient is gy scattered
            scat = torch.zeros_like(want["embedding.weight"]).index_add_(0, prob.idx, prob.gy.double())
            assert torch.equal(got["embedding.weight"].cpu().double(), scat)


# ---------------------------------------------------------------------------------------
# C. the fused step
# ---------------------------------------------------------------------------------------
def _run_engine(prob, *, lr, betas, in_batch=False, masks=True, **engine_kwargs):
    """One FusedTrainStep over prob.batches (injected negatives; injected keep masks unless
    masks=False: then the step draws them from its own stream).  Returns (model, opts, losses, eng)."""
    from gpu_helpers import ttamm_model_from, ttamm_optimizers

    model = ttamm_model_from(prob)
    opts = ttamm_optimizers(model, lr=lr, betas=betas)
    eng = ttamm.FusedTrainStep(model, opts, negatives_per_positive=prob.shape.N, positives=prob.positives,
                               user_features=prob.user_features.cuda(), item_features=prob.item_features.cuda(),
                               loss_weights=LOSS_WEIGHTS, max_batch=prob.shape.B, in_batch_negatives=in_batch,
                               **engine_kwargs)
    losses = []
    for (users, pos, neg, um, im) in prob.batches:
        km = {"user": [m.cuda() for m in um], "item": [m.cuda() for m in im]} if masks else None
        eng.step(users.cuda(), pos.cuda(), neg.cuda().reshape(-1) if prob.shape.N else None, keep_masks=km)
        losses.append(eng.last_losses())
    eng.finish()
    return model, opts, losses, eng


def _oracle_step(prob, *, in_batch: bool, dtype=torch.float32):
    """One oracle step at lr = 0, betas (0, 0.999) (exp_avg == the gradient); dtype float64: the same
    restatement with every parameter and feature row double."""
    model = clone_model(prob.model).to(dtype)
    opts = ref.build_optimizers(model, lr=1e-3, betas=(0.0, 0.999), weight_decay=0.01)
    set_lr(opts, 0.0)
    users, pos, neg, um, im = prob.batches[0]
    res = ref.train_step(model, opts, users, pos, neg, user_features=prob.user_features.to(dtype),
                         item_features=prob.item_features.to(dtype), loss_weights=LOSS_WEIGHTS,
                         user_keep_masks=um, item_keep_masks=im, in_batch=in_batch)
    return model, opts, res


def _grads(model, opts) -> dict:
    return {n: st["exp_avg"] for n, st in named_optimizer_state(model, opts).items()}


def _check_against_oracle(prob, tm, to, tl, *, in_batch=False, bf16=False) -> float:
    """test_step_gradients_match_oracle's assertions (losses and per-tensor rel_err at 1e-5; bf16
    towers at test_bf16_step_gradients_match_bf16_oracle's).  An fp32 tensor past 1e-5 is judged as
    test_fullsize_parity_gpu._compare judges it: against the oracle step re-run in float64, ttamm
    within 1e-5 of that or at least as close to it as the fp32 oracle is.  Returns the worst rel_err."""
    om, oo, ores = _oracle_step(prob, in_batch=in_batch)
    loss_tol = BF16_LOSS_TOL if bf16 else TOL
    for key in ("total", "bce") + (("mimic_user", "mimic_item") if prob.shape.mimic else ()):
        want = getattr(ores, key)
        assert abs(tl[key] - want) <= loss_tol * abs(want), (key, tl[key], want)
    og, tg = _grads(om, oo), _grads(tm, to)
    assert set(og) == set(tg)
    g64 = None
    worst = 0.0
    for name in sorted(og):
        err = rel_err(tg[name], og[name])
        if bf16:
            mean = ((tg[name].double().cpu() - og[name].double()).abs().mean()
                    / og[name].double().abs().max().clamp_min(1e-30)).item()
            assert err <= BF16_TOL, f"{name}: rel err {err:.3e}"
            assert mean <= BF16_MEAN_TOL, f"{name}: mean rel err {mean:.3e}"
        elif err > TOL:
            if g64 is None:
                m64, o64, _ = _oracle_step(prob, in_batch=in_batch, dtype=torch.float64)
                g64 = _grads(m64, o64)
            ours, theirs = rel_err(tg[name], g64[name]), rel_err(og[name], g64[name])
            print(f"  {name}: vs fp32 oracle {err:.2e}; vs float64: ttamm {ours:.2e}, fp32 oracle {theirs:.2e}")
            assert ours <= TOL or ours <= theirs, f"{name}: rel err {err:.3e} (vs float64 {ours:.3e} > {theirs:.3e})"
            err = ours
        worst = max(worst, err)
    for (n, p), (_, q) in zip(om.state_dict().items(), tm.state_dict().items()):  # lr = 0
        assert torch.equal(q.cpu(), p), n
    return worst


TILE_SHAPES = [
    Shape(U=50, I=300, F=37, D=12, B=40, N=3, hidden_dims=(100, 160, 200)),
    Shape(U=64, I=512, F=40, D=32, B=43, N=5, hidden_dims=(200,)),
    Shape(U=64, I=512, F=40, D=128, B=43, N=5, hidden_dims=(256,), gate_hidden=100),
]


@pytest.mark.parametrize("shape", TILE_SHAPES, ids=["w100-160-200", "w200", "w256-gate100"])
def test_step_tile_classes_match_oracle(shape, monkeypatch):
    """Layer widths in (96, 128), (128, 192) and (192, 256] on the default split-bf16 path: 128-wide
    tiles with a column tail, two column tiles with a tail, weight-gradient classes 2 (tail), 1, 3."""
    from gpu_helpers import run_ttamm

    _set_mode(monkeypatch, exact=False)
    prob = make_problem(shape, steps=1)
    tm, to, tres = run_ttamm(prob, lr=0.0, betas=(0.0, 0.999))
    worst = _check_against_oracle(prob, tm, to, tres[0])
    print(f"\ntile classes {shape.hidden_dims}: split mode worst rel_err {worst:.2e}")
    # the same widths on the pre-split-plane kernels (first layer: 128-wide with a tail, 128 x 2 with a
    # tail, 128 x 2) give the same gradients
    pm, po, pres = run_ttamm(prob, lr=0.0, betas=(0.0, 0.999), feature_planes=True)
    assert pres == tres
    g, gp = _grads(tm, to), _grads(pm, po)
    for n in g:
        assert torch.equal(g[n], gp[n]), f"feature_planes: {n}"


def _step_shapes():
    from test_step_parity_gpu import GATE_SHAPES

    odd = Shape(U=50, I=300, F=37, H=24, D=12, B=40, N=3, gate_hidden=20, hidden_dims=(24,))
    return {
        "tiny": (Shape(), False, False),
        "odd": (odd, False, False),
        "2hidden": (Shape(U=64, I=512, F=20, D=16, B=64, N=5, hidden_dims=(32, 24)), False, False),
        "concat": (Shape(fusion="concat"), False, False),
        "d96-c2dims-fused": (GATE_SHAPES[2], False, False),
        "d96-c2dims-generic": (GATE_SHAPES[2], False, True),
        "tile-classes": (TILE_SHAPES[0], False, False),
        "bf16-tiny": (Shape(matmul_dtype="bf16"), False, False),
        "bf16-odd": (Shape(**{**odd.__dict__, "matmul_dtype": "bf16"}), False, False),
        "inbatch-n0": (Shape(N=0), True, False),
        "inbatch-c2dims": (Shape(U=400, I=2000, F=605, H=192, D=96, B=300, N=5, hidden_dims=(192,)), True, False),
        "inbatch-d128-n0": (Shape(U=300, I=1500, F=40, H=64, D=128, B=200, N=0, hidden_dims=(64,)), True, False),
    }  # (shape, in-batch, generic gate)


STEP_IDS = ["tiny", "odd", "2hidden", "concat", "d96-c2dims-fused", "d96-c2dims-generic", "tile-classes", "bf16-tiny",
            "bf16-odd", "inbatch-n0", "inbatch-c2dims", "inbatch-d128-n0"]


@pytest.mark.parametrize("case", STEP_IDS)
def test_step_exact_mfma_matches_oracle(case, monkeypatch):
    """The fused step with TTAMM_FP32_MFMA=exact (gemm_kernel on v_mfma_f32_32x32x2_f32 for every
    forward, dgrad and weight gradient, inbatch_kernel for the in-batch block) against the oracle.
    On d96-c2dims the default path runs too: both pass and their gradients differ in at least one
    bit, or the variable did not reach the library."""
    shape, in_batch, generic = _step_shapes()[case]
    bf16 = shape.matmul_dtype == "bf16"
    prob = make_problem(shape, steps=1)
    _set_mode(monkeypatch, exact=True, generic=generic)
    tm, to, tl, _ = _run_engine(prob, lr=0.0, betas=(0.0, 0.999), in_batch=in_batch)
    worst = _check_against_oracle(prob, tm, to, tl[0], in_batch=in_batch, bf16=bf16)
    print(f"\n{case}: exact mode worst rel_err {worst:.2e}")
    if case == "d96-c2dims-fused":
        _set_mode(monkeypatch, exact=False, generic=generic)
        dm, do, dl, _ = _run_engine(prob, lr=0.0, betas=(0.0, 0.999), in_batch=in_batch)
        worst = _check_against_oracle(prob, dm, do, dl[0], in_batch=in_batch)
        eg, dg = _grads(tm, to), _grads(dm, do)
        bits = {n: _bits_differing(eg[n], dg[n]) for n in eg}
        total = sum(bits.values())
        print(f"{case}: split mode worst rel_err {worst:.2e}; bits differing between the split and the exact "
              f"run's gradients: {total} over {sum(1 for v in bits.values() if v)} of {len(bits)} tensors")
        assert total > 0, "TTAMM_FP32_MFMA=exact did not reach the library: both runs gave the same bits"


PLANE_SHAPES = {
    "f12": (Shape(), False),  # one partial k-tile
    "f16": (Shape(F=16), False),
    "f37": (Shape(U=50, I=300, F=37, H=24, D=12, B=40, N=3, gate_hidden=20, hidden_dims=(24,)), False),
    "f605-h192-d96": (Shape(U=96, I=768, F=605, H=192, D=96, B=37, N=5, hidden_dims=(192,)), False),  # classes 1, 0
    "f40-h128": (Shape(U=64, I=512, F=40, H=128, D=32, B=43, N=5, hidden_dims=(128,)), False),  # class 2
    "f40-h256": (Shape(U=64, I=512, F=40, H=256, D=32, B=43, N=5, hidden_dims=(256,)), False),  # class 3
    # F a multiple of the 128-row M tile: the weight gradient's ones column (the bias gradient) alone in
    # an M tile of its own, past the rows' planes
    "f128": (Shape(U=64, I=512, F=128, H=32, D=16, B=43, N=5, hidden_dims=(32,)), False),
    "concat": (Shape(fusion="concat"), False),
    "inbatch": (Shape(U=50, I=300, F=37, H=24, D=12, B=40, N=3, gate_hidden=20, hidden_dims=(24,)), True),
}


def _assert_same_run(a, b, what: str) -> None:
    (am, ao, al), (bm, bo, bl) = a, b
    assert al == bl, f"{what}: losses {al} != {bl}"
    for (n, p), (_, q) in zip(am.state_dict().items(), bm.state_dict().items()):
        assert torch.equal(p, q), f"{what}: {n}"
    sa, sb = named_optimizer_state(am, ao), named_optimizer_state(bm, bo)
    assert set(sa) == set(sb)
    for n in sa:
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(sa[n][k], sb[n][k]), f"{what}: {n} {k}"


@pytest.mark.parametrize("case", list(PLANE_SHAPES))
def test_feature_planes_same_bits(case, monkeypatch):
    """feature_planes=True (ttamm_to_planes, the pre-split A-operand forward kernels and the plane
    weight-gradient kernels) gives the default path's bits: two real steps, every parameter, both
    optimizer moments and the losses.  (The plane weight-gradient kernels first summed the bias
    gradient as a column sum of dY: the same values in another order than the default path's ones
    column, so the first layer's bias gradient differed in its last bits in every case here; they
    now stage the ones column in the hi plane.)  With
    TTAMM_FP32_MFMA=exact the planes are ignored (the documented fallback): planes on == exact alone."""
    shape, in_batch = PLANE_SHAPES[case]
    prob = make_problem(shape, steps=2)
    runs = {}
    for exact in (False, True):
        _set_mode(monkeypatch, exact=exact)
        for planes in (False, True):
            m, o, l, eng = _run_engine(prob, lr=1e-3, betas=(0.9, 0.999), in_batch=in_batch, feature_planes=planes)
            for desc in (eng.args.user, eng.args.item):
                assert bool(desc.features_planes) == planes
                assert not planes or desc.feat_planes_ld >= 48 * ((shape.F + 15) // 16)
            runs[exact, planes] = (m, o, l)
    _assert_same_run(runs[False, True], runs[False, False], "planes vs default")
    _assert_same_run(runs[True, True], runs[True, False], "exact + planes vs exact")
    # (the two switches are live: the exact run is not the split run)
    ga, gb = _grads(*runs[False, False][:2]), _grads(*runs[True, False][:2])
    assert any(not torch.equal(ga[n], gb[n]) for n in ga)


@pytest.mark.parametrize("shape", [Shape(dropout=0.3), Shape(dropout=0.3, hidden_dims=(100, 20))],
                         ids=["h16", "h100-20"])
def test_dropout_stream_is_kernel_independent(shape, monkeypatch):
    """The step's own dropout stream (no injected masks, a fixed seed) under the three forward
    kernels' epilogues: the planes run equals the default bit for bit; the exact run is within 2e-5
    (the two paths' 1e-5 bounds against the truth, summed) on losses and gradients — one differing
    keep-mask element moves them by orders of magnitude more."""
    prob = make_problem(shape, steps=1)
    kw = dict(lr=0.0, betas=(0.0, 0.999), masks=False, seed=20240607)
    _set_mode(monkeypatch, exact=False)
    dm, do, dl, _ = _run_engine(prob, **kw)
    pm, po, pl, _ = _run_engine(prob, feature_planes=True, **kw)
    _assert_same_run((pm, po, pl), (dm, do, dl), "planes vs default")
    _set_mode(monkeypatch, exact=True)
    em, eo, el, _ = _run_engine(prob, **kw)
    for key in ("total", "bce", "mimic_user", "mimic_item"):
        assert abs(el[0][key] - dl[0][key]) <= 2e-5 * abs(dl[0][key]), (key, el[0][key], dl[0][key])
    dg, eg = _grads(dm, do), _grads(em, eo)
    worst = max(rel_err(eg[n], dg[n]) for n in dg)
    print(f"\ndropout stream {shape.hidden_dims}: exact vs split worst rel_err {worst:.2e}")
    for n in dg:
        err = rel_err(eg[n], dg[n])
        assert err <= 2e-5, f"{n}: rel err {err:.3e}"
    # the masks are real: another seed gives another gradient
    _set_mode(monkeypatch, exact=False)
    om_, oo_, _, _ = _run_engine(prob, **{**kw, "seed": 20240608})
    assert max(rel_err(_grads(om_, oo_)[n], dg[n]) for n in dg) > 1e-3


# ---------------------------------------------------------------------------------------
# D. single ops
# ---------------------------------------------------------------------------------------
def _inbatch_inputs(B, Bc, D, row_base, scale=0.3):
    g = torch.Generator(device="cuda").manual_seed(B + Bc + D)
    users = torch.randn((B, D), device="cuda", generator=g) * scale
    pos = torch.randn((Bc, D), device="cuda", generator=g) * scale
    pos[row_base:row_base + B] += 0.5 * users
    return users, pos


@pytest.mark.parametrize("B,Bc,D,row_base", [(77, 77, 12, 0), (130, 130, 40, 0), (300, 300, 96, 0), (200, 900, 128, 450)],
                         ids=["dp32", "dp64", "dp96", "dp128"])
def test_inbatch_op_exact_mfma_matches_fp64(B, Bc, D, row_base, monkeypatch):
    """ttamm.inbatch_bce under TTAMM_FP32_MFMA=exact (inbatch.hip inbatch_kernel<32|64|96|128> by the
    padded D) against the chunked float64 definition, test_inbatch_op_gpu.py's 1e-5 bounds."""
    users, pos = _inbatch_inputs(B, Bc, D, row_base)
    inv = 1.0 / (max(B, Bc) * Bc)
    _set_mode(monkeypatch, exact=True)
    loss, du, dp = ttamm.inbatch_bce(users, pos, row_base=row_base, inv_count=inv)
    torch.cuda.synchronize()
    want_loss, want_du, want_dp = ref.inbatch_bce_chunked(users, pos, row_base=row_base, inv_count=inv)

    def rel(a, b):
        return float((a.double() - b).abs().max() / b.abs().max())

    print(f"\ninbatch exact D={D}: loss {abs(float(loss) - want_loss) / abs(want_loss):.2e}, "
          f"dU {rel(du, want_du):.2e}, dP {rel(dp, want_dp):.2e}")
    assert abs(float(loss) - want_loss) <= TOL * abs(want_loss), (float(loss), want_loss)
    assert rel(du, want_du) <= TOL and rel(dp, want_dp) <= TOL
    if (B, D) == (300, 96):
        _set_mode(monkeypatch, exact=False)
        _, du2, dp2 = ttamm.inbatch_bce(users, pos, row_base=row_base, inv_count=inv)
        torch.cuda.synchronize()
        assert rel(du2, want_du) <= TOL and rel(dp2, want_dp) <= TOL
        bits = _bits_differing(du, du2) + _bits_differing(dp, dp2)
        print(f"inbatch D=96: bits differing between the split and the exact kernel's gradients: {bits}")
        assert bits > 0, "TTAMM_FP32_MFMA=exact did not reach the in-batch kernel: both runs gave the same bits"


def _converter_inputs(rows: int, cols: int) -> torch.Tensor:
    """Finite fp32 values: randn x 10^U(-6, 3), with exact zeros, -0 and bf16 rounding ties
    (1 + odd / 256: halfway between two bf16 values) mixed in."""
    g = torch.Generator().manual_seed(1000 * rows + cols)
    x = torch.randn((rows, cols), generator=g) * torch.pow(10.0, torch.rand((rows, cols), generator=g) * 9.0 - 6.0)
    kind = torch.randint(0, 8, (rows, cols), generator=g)
    odd = 2.0 * torch.randint(0, 128, (rows, cols), generator=g).float() + 1.0
    x = torch.where(kind == 0, torch.zeros_like(x), x)
    x = torch.where(kind == 1, -torch.zeros_like(x), x)
    x = torch.where(kind == 2, (1.0 + odd / 256.0) * torch.where(odd % 3 == 0, -1.0, 1.0), x)
    if rows * cols >= 64:
        assert ((x == 0) & torch.signbit(x)).any() and (kind == 2).any()
    return x


def _src_layouts(x: torch.Tensor):
    """(name, device view of x, its row stride): packed rows, and rows inside a wider buffer whose
    other columns hold a finite value no output may show."""
    rows, cols = x.shape
    yield "packed", x.cuda().contiguous(), cols
    wide = torch.full((rows, cols + 5), 12345.0, device="cuda")
    wide[:, :cols] = x.cuda()
    yield "ld_src", wide[:, :cols], cols + 5


WIDTHS = [1, 15, 16, 17, 37, 605]
SENTINEL = 0x5A5A


@pytest.mark.parametrize("rows", [1, 1000])
@pytest.mark.parametrize("cols", WIDTHS)
def test_to_planes_layout_and_exact_sum(rows, cols):
    """ttamm_to_planes (to_planes_kernel): hi = bf16(x), mid = bf16(x - hi), lo with hi + mid + lo == x,
    at dst[r, 48 (c / 16) + {0, 16, 32} + c % 16] (ttamm.h); zero planes for cols <= c < 16 ceil(cols / 16);
    nothing written past 48 ceil(cols / 16) of a row."""
    lib = _lib.load()
    x = _converter_inputs(rows, cols)
    kc = (cols + 15) // 16
    hi = x.to(torch.bfloat16)
    mid = (x - hi.float()).to(torch.bfloat16)
    want = torch.zeros((rows, kc, 3, 16), dtype=torch.int16)
    c = torch.arange(cols)
    want[:, c // 16, 0, c % 16] = hi.view(torch.int16)
    want[:, c // 16, 1, c % 16] = mid.view(torch.int16)
    stream = _lib.stream_handle(torch.device("cuda"))
    layouts = [(name, src, ld_src, 48 * kc) for name, src, ld_src in _src_layouts(x)]
    layouts.append(("ld_dst", x.cuda().contiguous(), cols, 48 * kc + 24))
    for name, src, ld_src, ld_dst in layouts:
        dst = torch.full((rows, ld_dst), SENTINEL, dtype=torch.int16, device="cuda")
        _lib.check(lib.ttamm_to_planes(src.data_ptr(), rows, cols, ld_src, dst.data_ptr(), ld_dst, stream))
        torch.cuda.synchronize()
        got = dst.cpu()
        assert (got[:, 48 * kc:] == SENTINEL).all(), f"{name}: wrote past 48 ceil(cols / 16)"
        planes = got[:, : 48 * kc].reshape(rows, kc, 3, 16)
        assert torch.equal(planes[:, :, 0], want[:, :, 0]), f"{name}: hi plane"
        assert torch.equal(planes[:, :, 1], want[:, :, 1]), f"{name}: mid plane"
        vals = planes.view(torch.bfloat16).double()  # [rows, kc, 3, 16]
        total = vals.sum(dim=2).reshape(rows, kc * 16)  # |hi| >> |mid| >> |lo|: exact in float64
        assert torch.equal(total[:, :cols], x.double()), f"{name}: hi + mid + lo != x"
        assert (planes.permute(0, 1, 3, 2).reshape(rows, kc * 16, 3)[:, cols:] == 0).all(), f"{name}: padded columns"
    dst = torch.zeros((rows, 48 * kc + 8), dtype=torch.int16, device="cuda")
    src = x.cuda().contiguous()
    for bad in (48 * kc - 8, 48 * kc + 4):  # too short; not a multiple of 8
        with pytest.raises(ValueError, match="to_planes"):
            _lib.check(lib.ttamm_to_planes(src.data_ptr(), rows, cols, cols, dst.data_ptr(), bad, stream))
    assert not dst.any()


@pytest.mark.parametrize("rows", [1, 1000])
@pytest.mark.parametrize("cols", WIDTHS)
def test_to_bf16_matches_torch(rows, cols):
    """ttamm_to_bf16 (to_bf16_kernel) == .to(torch.bfloat16) bit for bit; columns cols..ld_dst zero."""
    lib = _lib.load()
    x = _converter_inputs(rows, cols)
    want = x.to(torch.bfloat16).view(torch.int16)
    stream = _lib.stream_handle(torch.device("cuda"))
    layouts = [(name, src, ld_src, (cols + 7) // 8 * 8) for name, src, ld_src in _src_layouts(x)]
    layouts.append(("ld_dst", x.cuda().contiguous(), cols, (cols + 7) // 8 * 8 + 16))
    layouts.append(("ld_dst == cols", x.cuda().contiguous(), cols, cols))
    for name, src, ld_src, ld_dst in layouts:
        dst = torch.full((rows, ld_dst), SENTINEL, dtype=torch.int16, device="cuda")
        _lib.check(lib.ttamm_to_bf16(src.data_ptr(), rows, cols, ld_src, dst.data_ptr(), ld_dst, stream))
        torch.cuda.synchronize()
        got = dst.cpu()
        assert torch.equal(got[:, :cols], want), name
        assert (got[:, cols:] == 0).all(), f"{name}: columns past cols"
    with pytest.raises(ValueError, match="to_bf16"):
        _lib.check(lib.ttamm_to_bf16(src.data_ptr(), rows, cols, cols, dst.data_ptr(), cols - 1, stream))
