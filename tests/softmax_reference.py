"""The definition of ttamm's in-batch softmax objective, for the tests (not a test itself).

With S = U P^T [B, Bc], temperature t > 0 and user b's own positive at column row_base + b:

    lse_b    = log sum_j exp(S_bj / t)
    loss_sum = sum_b (lse_b - S_{b,row_base+b} / t)          L = inv_count * loss_sum
    dS_bj    = (exp(S_bj / t - lse_b) - [j == row_base + b]) * inv_count / t
    dU = dS P, dP = dS^T U

``inbatch_softmax_chunked`` evaluates it in the manner of oracle.cpu_reference.inbatch_bce_chunked;
``train_step_softmax`` restates oracle.cpu_reference.train_step with that retrieval term, from the
oracle's own blocks."""

from __future__ import annotations

from typing import Mapping, Sequence

import torch
import torch.nn.functional as F

from oracle import cpu_reference as ref


def inbatch_softmax_chunked(users: torch.Tensor, positives: torch.Tensor, *, row_base: int = 0,
                            temperature: float = 1.0, inv_count: float | None = None, chunk: int = 1024,
                            dtype: torch.dtype = torch.float64) -> tuple[float, torch.Tensor, torch.Tensor]:
    """(loss_sum, dL/dusers, dL/dpositives) for L = inv_count * loss_sum (default 1 / B), evaluated
    in ``dtype``, ``chunk`` users at a time so a large score matrix is never held whole.  Runs on
    whatever device the inputs are on."""
    u = users.to(dtype)
    p = positives.to(dtype)
    B = u.shape[0]
    if inv_count is None:
        inv_count = 1.0 / B
    loss = 0.0
    du = torch.empty_like(u)
    dp = torch.zeros_like(p)
    for lo in range(0, B, chunk):
        hi = min(B, lo + chunk)
        z = (u[lo:hi] @ p.t()) / temperature
        rows = torch.arange(hi - lo, device=z.device)
        cols = row_base + lo + rows
        lse = torch.logsumexp(z, dim=1)
        loss += float((lse - z[rows, cols]).sum().item())
        ds = torch.exp(z - lse[:, None])
        ds[rows, cols] -= 1.0
        ds *= inv_count / temperature
        du[lo:hi] = ds @ p
        dp += ds.t() @ u[lo:hi]
    return loss, du, dp


def train_step_softmax(
    model: ref.OracleModel,
    optimizers: Sequence[torch.optim.Optimizer],
    users: torch.Tensor,
    pos_items: torch.Tensor,
    *,
    temperature: float,
    user_features: torch.Tensor | None,
    item_features: torch.Tensor | None,
    loss_weights: Mapping[str, float] | None = None,
    user_keep_masks: Sequence[torch.Tensor] | None = None,
    item_keep_masks: Sequence[torch.Tensor] | None = None,
    train: bool = True,
) -> ref.StepResult:
    """oracle.cpu_reference.train_step(in_batch=True) with no sampled negatives and the retrieval
    term F.cross_entropy((u @ p^T) / temperature, arange(B)); the mimic MSEs, the total and the
    optimizer steps as there.  ``train=False``: the eval-mode losses of the batch (dropout off, no
    backward, no optimizer step), the definition of the validation pass."""
    model.train(train)
    lw = dict(loss_weights or {})
    lam_u = float(lw.get("mimic_user", 0.0))
    lam_i = float(lw.get("mimic_item", 0.0))
    mimic = model.adaptive_mimic
    B = users.shape[0]
    if train:
        for opt in optimizers:
            opt.zero_grad()
    uf = user_features.index_select(0, users) if user_features is not None and user_features.numel() else None
    pf = item_features.index_select(0, pos_items) if item_features is not None and item_features.numel() else None
    t_u = ref.tower_forward(model.user_encoder, users, uf, user_keep_masks if train else None)
    t_p = ref.tower_forward(model.item_encoder, pos_items, pf, item_keep_masks if train else None)
    loss_u = loss_i = None
    if mimic is not None:
        u, a_u = ref.gather_aug(mimic.user_augmented, users, t_u)
        p, a_p = ref.gather_aug(mimic.item_augmented, pos_items, t_p)
        loss_u = F.mse_loss(a_u, t_p.detach())
        loss_i = F.mse_loss(a_p, t_u.detach())
    else:
        u, p = t_u, t_p
    ce = F.cross_entropy((u @ p.t()) / temperature, torch.arange(B))
    total = ce
    if loss_u is not None and lam_u > 0:
        total = total + lam_u * loss_u
    if loss_i is not None and lam_i > 0:
        total = total + lam_i * loss_i
    if train:
        total.backward()
        for opt in optimizers:
            opt.step()
    return ref.StepResult(
        float(total.item()), float(ce.item()),
        float(loss_u.item()) if loss_u is not None else 0.0,
        float(loss_i.item()) if loss_i is not None else 0.0,
    )
