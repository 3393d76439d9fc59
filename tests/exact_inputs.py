"""Exact-arithmetic tower problems: inputs on a fixed binary grid whose every product and every
partial sum of every GEMM of the tower's forward and backward is exactly representable in fp32.
The result then does not depend on the summation order, the tile, the split-K chunking or the
operand split, so a correct kernel must reproduce the float64 value bit for bit: one dropped,
duplicated or mis-indexed element, column tail, k tail, chunk or plane changes bits.

The tower is linear + ReLU only (fusion "sum" or "concat", no dropout, no gate: a sigmoid is not
exact), its ID table dense, the upstream gradient ``gy`` given.  Recipes:

  int        features in {-2..2}, weights in {-1, 0, 1}, biases in {-2..2}, ID rows in {-3..3},
             gy in {-1, 1}: integers leave the mid and lo planes of the bf16 split at zero
  x3         one Linear; features a + b/256 + c/65536 (a in {-1, 0, 1}, b, c in {-3..3}): the
             A operand's hi, mid and lo planes are all non-zero
  w3         the same grid on the first layer's weights, integer features (the B operand's planes)
  mm         features and first-layer weights both a + b/256: the mid x mid product
  w2-dgrad   one hidden layer, the second layer's weights a + b/256: the K-major B operand's mid
             plane in dgrad

``reference()`` restates the tower in float64 GEMM by GEMM (with ``bf16=True``: both operands of
every product rounded to bf16, the definition of oracle.cpu_reference._BF16Linear) and returns,
beside the output and the gradients, the precondition that makes the comparison order-free:

  for every GEMM C = A B (+ bias):  max_ij (sum_k |a_ik| |b_kj| + |bias_j|) / (lsb_A lsb_B) < 2^23

with lsb_X the largest power of two dividing every entry of X.  Every partial sum, in any order and
of any subset of the terms, is then a multiple of lsb_A lsb_B below 2^23 of them: exact in fp32's
24-bit significand, with one bit to spare because the three planes of a split operand can sum to
slightly more than |x| in absolute value (|hi| + |mid| + |lo| <= |x| (1 + 2^-7)).  It also checks
that every float64 result equals its own fp32 rounding."""

from __future__ import annotations

from dataclasses import dataclass, field

import torch
from torch import nn

from helpers import Shape, make_problem

LIMIT = float(2 ** 23)
RECIPES = ("int", "x3", "w3", "mm", "w2-dgrad")


@dataclass
class ExactCase:
    shape: Shape
    rows: tuple  # the R of each tower call of the case
    recipe: str = "int"


def _shape(F, hidden, D, **kw) -> Shape:
    kw.setdefault("fusion", "sum")
    return Shape(U=2, I=2, F=F, H=hidden[0] if hidden else D, D=D, B=2, N=1, hidden_dims=tuple(hidden), dropout=0.0,
                 sparse=False, mimic=False, **kw)


# F -> hidden -> D and the rows R of the tower call.  The tile classes follow gemm.hip pick_tile_n
# (forward / dgrad output tile width; every launch here has < 300 wide tiles or is a dgrad, so the
# narrow set {96, 128}, unless stated) and wgrad_class (0: 96-wide, 1: 192, 2: 128, 3: 128 at
# multiples of 256) of the layer's output width.
CASES: dict[str, ExactCase] = {
    # forward 24 and 12 wide: the 96-wide tile; K = 37 (two full k-tiles and a tail of 5, lda padded to
    # 40); rows 129 = one full 128-row block and a block with one row; wgrad class 0 for both layers;
    # N = 12: one 8-column epilogue group and a half one
    "narrow": ExactCase(_shape(37, (24,), 12), (129,)),
    # forward N = 100: one 128-wide tile with 28 padded columns; 160: 96 x 2 (tail 64); 200: 128 x 2
    # (tail 72); 12: 96.  wgrad classes by output width: 100 -> 2 (128 with a tail), 160 -> 1 (192),
    # 200 -> 3 (256 = 128 x 2, tail 72), 12 -> 0.  dgrad at K = 12, 200, 160 with N = 200, 160, 100
    "classes": ExactCase(_shape(37, (100, 160, 200), 12), (257,)),
    # K = 605 = 37 k-tiles of 16 and a tail of 13; forward N = 192: 96 x 2, N = 96: 96; wgrad classes 1
    # (192) and 0 (96); 300 rows = three split-K chunks at the smallest rows per split (128)
    "c2dims": ExactCase(_shape(605, (192,), 96), (300,)),
    # widths 256, 128, 128 and the concat projection 256 -> 128: 128-wide tiles without tails; wgrad
    # classes 3 (256) and 2 (128); the projection GEMM and its dgrad at K = 256 / N = 256
    "c4dims": ExactCase(_shape(605, (256, 128), 128, fusion="concat", concat_out=128), (385,)),
    # 35 row blocks x 10 column tiles of 192 = 350 wide tiles (>= 300): the 192-wide forward tile;
    # wgrad class 1 with ten column tiles; dgrad K = 8
    "wide192": ExactCase(_shape(16, (1920,), 8), (4480,)),
    # a block with one valid row; one short split-K chunk (127 rows)
    "one-row": ExactCase(_shape(40, (64,), 32), (1, 127)),
    # the planes of each operand (96-wide tiles, wgrad class 0)
    "x3": ExactCase(_shape(40, (), 32, feature_type="linear"), (64,), "x3"),
    "w3": ExactCase(_shape(40, (), 32, feature_type="linear"), (64,), "w3"),
    "mm": ExactCase(_shape(16, (), 8, feature_type="linear"), (64,), "mm"),
    "w2-dgrad": ExactCase(_shape(40, (64,), 32), (64,), "w2-dgrad"),
}
PLANE_CASES = ("x3", "w3", "mm", "w2-dgrad")


@dataclass
class ExactProblem:
    shape: Shape
    recipe: str
    tower: nn.Module  # the oracle's item tower (fp32 parameters on the grid)
    idx: torch.Tensor  # [R] int64
    feats: torch.Tensor  # [R, F] fp32, one row per index
    gy: torch.Tensor  # [R, P] fp32


@dataclass
class Precondition:
    """max_ij (sum_k |a_ik||b_kj| + |bias_j|) / (lsb_A lsb_B) per GEMM, and the float64 results that
    are not their own fp32 rounding."""
    bounds: dict = field(default_factory=dict)
    inexact: list = field(default_factory=list)

    @property
    def worst(self) -> float:
        return max(self.bounds.values())

    @property
    def ok(self) -> bool:
        return bool(self.bounds) and self.worst < LIMIT and not self.inexact

    def __str__(self) -> str:
        name = max(self.bounds, key=self.bounds.get)
        return f"worst GEMM {name}: {self.worst:.0f} of {LIMIT:.0f}; not fp32-exact: {self.inexact}"


def _ints(gen, shape, lo, hi, nonzero=False) -> torch.Tensor:
    v = torch.randint(lo, hi + 1, shape, generator=gen).float()
    if nonzero:
        v = torch.where(v == 0, torch.ones_like(v), v)
    return v


def _grid3(gen, shape, planes: int) -> torch.Tensor:
    """a + b/256 (+ c/65536), a in {-1, 0, 1}, b, c in {-3..3}; b and c never zero, so every element
    reaches its mid (and lo) plane."""
    v = _ints(gen, shape, -1, 1) + _ints(gen, shape, -3, 3, nonzero=True) / 256.0
    if planes == 3:
        v = v + _ints(gen, shape, -3, 3, nonzero=True) / 65536.0
    return v


def _linears(tower) -> list[nn.Linear]:
    net = tower.feature_encoder.network
    return [net] if isinstance(net, nn.Linear) else [m for m in net if isinstance(m, nn.Linear)]


def build(shape: Shape, R: int, recipe: str = "int", *, seed: int = 7) -> ExactProblem:
    """The exact problem of ``shape`` at R tower rows: helpers.make_problem's model with every
    parameter of the item tower, the feature rows and gy overwritten by grid values."""
    assert shape.fusion in ("sum", "concat") and shape.activation == "relu" and shape.dropout == 0.0
    assert not shape.sparse and not shape.mimic and recipe in RECIPES
    # every table row is looked up 3 times (odd: with gy in {-1, 1} its gradient entries are never 0)
    I = max(1, R // 3)
    shape = Shape(**{**shape.__dict__, "I": I})
    tower = make_problem(shape, steps=0).model.item_encoder
    gen = torch.Generator().manual_seed(seed + 1000 * R + len(recipe))
    lin = _linears(tower)
    F, P = shape.F, shape.P
    with torch.no_grad():
        tower.embedding.weight.copy_(_ints(gen, (I, shape.D), -3, 3))
        for m in lin:
            m.weight.copy_(_ints(gen, tuple(m.weight.shape), -1, 1))
            m.bias.copy_(_ints(gen, tuple(m.bias.shape), -2, 2))
        if shape.fusion == "concat":
            tower.projection.weight.copy_(_ints(gen, tuple(tower.projection.weight.shape), -1, 1))
            tower.projection.bias.copy_(_ints(gen, tuple(tower.projection.bias.shape), -2, 2))
        feats = _ints(gen, (R, F), -2, 2)
        if recipe == "x3":
            feats = _grid3(gen, (R, F), 3)
        elif recipe == "w3":
            lin[0].weight.copy_(_grid3(gen, tuple(lin[0].weight.shape), 3))
        elif recipe == "mm":
            feats = _grid3(gen, (R, F), 2)
            lin[0].weight.copy_(_grid3(gen, tuple(lin[0].weight.shape), 2))
        elif recipe == "w2-dgrad":
            lin[1].weight.copy_(_grid3(gen, tuple(lin[1].weight.shape), 2))
        gy = _ints(gen, (R, P), -1, 1, nonzero=True)
        if R < 16:
            # a handful of rows: without help half the hidden units are inactive and most gradient
            # entries zero.  Non-zero features; each first-layer row's sign set so that the unit is
            # active on row 0; the last layer's first output row zeroed so that each hidden unit's
            # gradient sums an odd number of +-1 terms (never 0)
            feats = _ints(gen, (R, F), -2, 2, nonzero=True)
            if len(lin) > 1:
                w, b = lin[0].weight, lin[0].bias
                pre = feats[0] @ w.t()
                w.mul_(torch.where(pre < 0, -1.0, 1.0).unsqueeze(1))
                b.copy_(torch.where(pre.abs() + b <= 0, torch.ones_like(b), b))
                lin[-1].weight.copy_(_ints(gen, tuple(lin[-1].weight.shape), -1, 1, nonzero=True))
                lin[-1].weight[0].zero_()
    idx = torch.arange(I).repeat_interleave(3)[:R]
    idx = torch.cat([idx, torch.zeros(R - idx.numel(), dtype=torch.long)])
    idx = idx[torch.randperm(R, generator=gen)]
    return ExactProblem(shape, recipe, tower, idx, feats, gy)


def _lsb(t: torch.Tensor) -> float:
    """The largest power of two that divides every entry of t (float64; 1 for an all-zero tensor)."""
    nz = t[t != 0]
    if nz.numel() == 0:
        return 1.0
    m, e = torch.frexp(nz)
    mant = (m.abs() * float(2 ** 53)).to(torch.int64)  # exact: 53-bit significands
    low = (mant & -mant).double()  # the lowest set bit of each significand
    return float((low * torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 53).double())).min())


def _bf(x: torch.Tensor) -> torch.Tensor:
    x32 = x.float()
    assert torch.equal(x32.double(), x), "bf16 restatement: a float64 value that is not an fp32 one"
    return x32.to(torch.bfloat16).double()


def reference(prob: ExactProblem, *, bf16: bool = False) -> tuple[torch.Tensor, dict, Precondition]:
    """(output, {parameter name: gradient}, precondition), all float64: the tower's training forward
    on (idx, feats) and the backward of gy, GEMM by GEMM.  bf16: every product's two operands rounded
    to bf16 first, the bias gradient the column sum of the rounded dy (oracle _BF16Linear)."""
    t = prob.tower
    names = {id(p): n for n, p in t.named_parameters()}
    rnd = _bf if bf16 else (lambda v: v)
    pc = Precondition()
    grads: dict[str, torch.Tensor] = {}

    def gemm(name, a, b, bias=None):
        a, b = rnd(a), rnd(b)
        c = a @ b
        mag = a.abs() @ b.abs()
        if bias is not None:
            c = c + bias
            mag = mag + bias.abs()
        pc.bounds[name] = float(mag.max()) / (_lsb(a) * _lsb(b))
        if not torch.equal(c.float().double(), c):
            pc.inexact.append(name)
        return c

    def linear_backward(tag, m, x, dy, need_dx):
        grads[names[id(m.weight)]] = gemm(f"{tag}.wgrad", dy.t(), x)
        grads[names[id(m.bias)]] = gemm(f"{tag}.bgrad", torch.ones((1, dy.shape[0]), dtype=torch.float64), dy)[0]
        return gemm(f"{tag}.dgrad", dy, m.weight.detach().double()) if need_dx else None

    lin = _linears(t)
    gy = prob.gy.double()
    x = prob.feats.double()
    acts, pre = [], []
    for l, m in enumerate(lin):
        acts.append(x)
        y = gemm(f"linear{l}.forward", x, m.weight.detach().double().t(), m.bias.detach().double())
        pre.append(y)
        x = torch.relu(y) if l + 1 < len(lin) else y
    f = x
    e = t.embedding.weight.detach().double()[prob.idx]
    if t.fusion == "sum":
        out = e + f
        de = df = gy
    else:
        ef = torch.cat([e, f], dim=1)
        p = t.projection
        out = gemm("projection.forward", ef, p.weight.detach().double().t(), p.bias.detach().double())
        d_ef = linear_backward("projection", p, ef, gy, True)
        de, df = d_ef[:, : e.shape[1]], d_ef[:, e.shape[1]:]
    if not torch.equal(out.float().double(), out):
        pc.inexact.append("output")
    dy = df
    for l in reversed(range(len(lin))):
        if l + 1 < len(lin):
            dy = dy * (pre[l] > 0)  # torch's ReLU backward: zero at 0
        dy = linear_backward(f"linear{l}", lin[l], acts[l], dy, l > 0)
    d_emb = torch.zeros_like(t.embedding.weight, dtype=torch.float64).index_add_(0, prob.idx, de)
    grads[names[id(t.embedding.weight)]] = d_emb
    for n, g in grads.items():
        if not torch.equal(g.float().double(), g):
            pc.inexact.append(n)
    return out, grads, pc
