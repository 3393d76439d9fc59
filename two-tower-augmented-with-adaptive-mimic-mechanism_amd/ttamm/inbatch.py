"""In-batch negatives as one op (ttamm's in-batch mode, BASELINE configs C2 / C4).

The reference scores sampled negatives only (training.py:770-798); the in-batch definition is
ttamm's own (oracle/cpu_reference.py train_step(in_batch=True)): every user is scored against
every positive of the (global) batch, label 1 on its own positive.  ``inbatch_bce`` runs the
fused kernel the training step uses (libttamm ``ttamm_inbatch_bce``, inbatch_x_kernel on
split-bf16 MFMA; nothing batch x n_positives is stored); ``inbatch_bce_loss`` runs its forward
third alone (``ttamm_inbatch_bce_loss``, inbatch_loss_kernel): the BCE sum without gradients.

``inbatch_softmax`` / ``inbatch_softmax_loss`` are the same pair for the softmax cross-entropy over
each user's row of S / temperature (``ttamm_inbatch_softmax``, ``ttamm_inbatch_softmax_loss``): a row
log-sum-exp pass that owns the loss, then the gradient kernel; no duplicate-item masking and no
logQ correction."""

from __future__ import annotations

import math

import torch

from . import _lib


def _check_rows(users: torch.Tensor, positives: torch.Tensor, row_base: int) -> tuple[torch.Tensor, torch.Tensor]:
    """The argument checks of both ops: contiguous float32 users [B, D] and positives [Bc, D] on
    the device, every user's own positive inside ``positives``."""
    _lib.require_rocm(users, "inbatch_bce")
    if users.dim() != 2 or positives.dim() != 2 or users.shape[1] != positives.shape[1]:
        raise ValueError("inbatch_bce: users [B, D] and positives [Bc, D] with one D")
    if users.dtype != torch.float32 or positives.dtype != torch.float32:
        raise ValueError("inbatch_bce: float32 rows")
    if not 0 <= row_base or row_base + users.shape[0] > positives.shape[0]:
        raise ValueError("inbatch_bce: every user's own positive must lie in positives (row_base + B <= Bc)")
    return users.contiguous(), positives.contiguous()


def inbatch_bce(users: torch.Tensor, positives: torch.Tensor, *, row_base: int = 0,
                inv_count: float | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """S = users @ positives.T with Y(b, row_base + b) = 1.  Returns (the BCE-with-logits sum over
    S as a float64 device scalar, dL/dusers, dL/dpositives) for L = inv_count * that sum
    (inv_count default 1 / S.numel(), the BCE mean)."""
    users, positives = _check_rows(users, positives, row_base)
    B, D = users.shape
    Bc = positives.shape[0]
    if inv_count is None:
        inv_count = 1.0 / float(B * Bc)
    lib = _lib.load()
    dev = users.device
    d_users = torch.empty_like(users)
    d_pos = torch.empty_like(positives)
    loss = torch.empty((), dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.ttamm_inbatch_workspace_size(B, Bc, D)), dtype=torch.uint8, device=dev)
    _lib.check(lib.ttamm_inbatch_bce(users.data_ptr(), B, users.stride(0), positives.data_ptr(), Bc,
                                     positives.stride(0), D, int(row_base), float(inv_count), d_users.data_ptr(),
                                     D, d_pos.data_ptr(), D, loss.data_ptr(), ws.data_ptr(), ws.numel(),
                                     _lib.stream_handle(dev)))
    return loss, d_users, d_pos


def inbatch_bce_loss(users: torch.Tensor, positives: torch.Tensor, *, row_base: int = 0) -> torch.Tensor:
    """The BCE-with-logits sum over S = users @ positives.T with Y(b, row_base + b) = 1, as a
    float64 device scalar: ``inbatch_bce(...)[0]`` without the gradients (libttamm
    ``ttamm_inbatch_bce_loss``, the forward-only inbatch_loss_kernel; the validation loss of
    in-batch mode).  Same argument checks as ``inbatch_bce``."""
    users, positives = _check_rows(users, positives, row_base)
    B, D = users.shape
    Bc = positives.shape[0]
    lib = _lib.load()
    dev = users.device
    loss = torch.empty((), dtype=torch.float64, device=dev)
    ws = torch.empty(max(int(lib.ttamm_inbatch_loss_workspace_size(B, Bc, D)), 4), dtype=torch.uint8, device=dev)
    _lib.check(lib.ttamm_inbatch_bce_loss(users.data_ptr(), B, users.stride(0), positives.data_ptr(), Bc,
                                          positives.stride(0), D, int(row_base), loss.data_ptr(), ws.data_ptr(),
                                          ws.numel(), _lib.stream_handle(dev)))
    return loss


def _inv_temperature(temperature: float) -> float:
    t = float(temperature)
    if not math.isfinite(t) or t <= 0.0:
        raise ValueError("inbatch_softmax: temperature must be finite and greater than zero")
    return 1.0 / t


def inbatch_softmax(users: torch.Tensor, positives: torch.Tensor, *, row_base: int = 0, temperature: float = 1.0,
                    inv_count: float | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """S = users @ positives.T, user b's own positive at column row_base + b.  Returns (the sum over
    the users of logsumexp(S[b] / temperature) - S[b, row_base + b] / temperature as a float64 device
    scalar, dL/dusers, dL/dpositives) for L = inv_count * that sum (inv_count default 1 / B, the
    cross-entropy mean)."""
    inv_t = _inv_temperature(temperature)
    users, positives = _check_rows(users, positives, row_base)
    B, D = users.shape
    Bc = positives.shape[0]
    if inv_count is None:
        inv_count = 1.0 / float(B)
    lib = _lib.load()
    dev = users.device
    d_users = torch.empty_like(users)
    d_pos = torch.empty_like(positives)
    loss = torch.empty((), dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.ttamm_inbatch_softmax_workspace_size(B, Bc, D)), dtype=torch.uint8, device=dev)
    _lib.check(lib.ttamm_inbatch_softmax(users.data_ptr(), B, users.stride(0), positives.data_ptr(), Bc,
                                         positives.stride(0), D, int(row_base), float(inv_count), inv_t,
                                         d_users.data_ptr(), D, d_pos.data_ptr(), D, loss.data_ptr(), ws.data_ptr(),
                                         ws.numel(), _lib.stream_handle(dev)))
    return loss, d_users, d_pos


def inbatch_softmax_loss(users: torch.Tensor, positives: torch.Tensor, *, row_base: int = 0,
                         temperature: float = 1.0) -> torch.Tensor:
    """``inbatch_softmax(...)[0]`` without the gradients: the log-sum-exp pass alone (libttamm
    ``ttamm_inbatch_softmax_loss``; the validation loss of the softmax objective), the same bits as
    the training op's loss.  Same argument checks as ``inbatch_softmax``."""
    inv_t = _inv_temperature(temperature)
    users, positives = _check_rows(users, positives, row_base)
    B, D = users.shape
    Bc = positives.shape[0]
    lib = _lib.load()
    dev = users.device
    loss = torch.empty((), dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.ttamm_inbatch_softmax_loss_workspace_size(B, Bc, D)), dtype=torch.uint8, device=dev)
    _lib.check(lib.ttamm_inbatch_softmax_loss(users.data_ptr(), B, users.stride(0), positives.data_ptr(), Bc,
                                              positives.stride(0), D, int(row_base), inv_t, loss.data_ptr(),
                                              ws.data_ptr(), ws.numel(), _lib.stream_handle(dev)))
    return loss
