"""CPU / fp32-reference sparse optimizer applies on EV slots.

These are the semantics the fused HIP applies (ops/hip/ev_apply_kernels.hip:
k_sparse_apply<Rule>, one rule struct per function here) must reproduce;
GPU numerics tests compare against this module.

Reference kernels: kernels/training_ali_ops.cc (CPU) and
training_ali_ops_gpu.cu.cc (kv_sparse_apply_{adagrad,ftrl,adam_async}).
All applies take the slot indices from the step's single hash probe and
skip un-admitted keys (slot < 0).
"""
from __future__ import annotations

import torch

from deeprec_amd.ops.common import bias_corrected_lr, optimizer_slabs


def _adm(storage, slots, grad):
    mask = slots >= 0
    return slots[mask].long(), grad[mask].float()


def _second_moment(v, s, g, beta2):
    vn = beta2 * v[s] + (1 - beta2) * g * g
    v[s] = vn
    return vn


def _adam_step(storage, rule, s, g, lr_t, beta1, beta2, epsilon):
    """Updates both moments; returns what the values move by."""
    m, v = optimizer_slabs(storage, rule, {})
    mn = beta1 * m[s] + (1 - beta1) * g
    vn = _second_moment(v, s, g, beta2)
    m[s] = mn
    return lr_t * mn / (vn.sqrt() + epsilon)


def _adagrad_step(storage, s, g, a, lr, epsilon):
    """a: the accumulator after this gradient."""
    storage.values[s] -= lr * g / (a.sqrt() + epsilon)


def apply_sgd(storage, slots, grad, lr, **_):
    s, g = _adm(storage, slots, grad)
    storage.values[s] -= lr * g


def apply_adagrad(storage, slots, grad, lr, initial_accumulator=0.1,
                  epsilon=0.0, **_):
    s, g = _adm(storage, slots, grad)
    accum, = optimizer_slabs(
        storage, "adagrad", dict(initial_accumulator=initial_accumulator))
    a = accum[s] + g * g
    accum[s] = a
    _adagrad_step(storage, s, g, a, lr, epsilon)


def apply_adagrad_decay(storage, slots, grad, lr, global_step,
                        initial_accumulator=0.1,
                        accumulator_decay_step=100000,
                        accumulator_decay_rate=0.9,
                        accumulator_baseline=0.0, epsilon=0.0, **_):
    """Periodically-decayed Adagrad (reference: AdagradDecayOptimizer,
    python/training/adagrad_decay.py): every accumulator_decay_step global
    steps the accumulator is multiplied by accumulator_decay_rate, floored
    at accumulator_baseline. Per-key decay bookkeeping lives in a 1-wide
    slab so sparsely-touched keys decay by the right number of periods."""
    s, g = _adm(storage, slots, grad)
    accum, period_slab = optimizer_slabs(
        storage, "adagrad_decay",
        dict(initial_accumulator=initial_accumulator))
    cur_period = float(global_step // max(1, accumulator_decay_step))
    dp = (cur_period - period_slab[s, 0]).clamp(min=0)
    decay = torch.pow(torch.tensor(accumulator_decay_rate), dp).unsqueeze(1)
    a = (accum[s] * decay).clamp(min=accumulator_baseline) + g * g
    accum[s] = a
    period_slab[s, 0] = cur_period
    _adagrad_step(storage, s, g, a, lr, epsilon)


def apply_adam(storage, slots, grad, lr, step_t, beta1=0.9, beta2=0.999,
               epsilon=1e-8, **_):
    """step_t: 1-based global apply count for bias correction."""
    s, g = _adm(storage, slots, grad)
    lr_t = bias_corrected_lr(lr, beta1 ** step_t, beta2 ** step_t)
    storage.values[s] -= _adam_step(storage, "adam", s, g, lr_t, beta1,
                                    beta2, epsilon)


def apply_adam_async(storage, slots, grad, lr, beta1_power, beta2_power,
                     beta1=0.9, beta2=0.999, epsilon=1e-8,
                     sparse_rmsprop=False, **_):
    """Lock-free async Adam (reference: AdamAsyncOptimizer,
    python/training/adam_async.py:40 and
    training_ali_ops_gpu.cu.cc:KvSparseApplyAdamAsyncKernel). beta powers
    are per-variable scalars maintained by the caller. With sparse_rmsprop
    the m accumulator is skipped and v behaves like RMSProp."""
    s, g = _adm(storage, slots, grad)
    if sparse_rmsprop:
        v, = optimizer_slabs(storage, "rmsprop", {})
        vn = _second_moment(v, s, g, beta2)
        storage.values[s] -= lr * g / (vn.sqrt() + epsilon)
        return
    lr_t = bias_corrected_lr(lr, beta1_power, beta2_power)
    storage.values[s] -= _adam_step(storage, "adam_async", s, g, lr_t,
                                    beta1, beta2, epsilon)


def apply_adamw(storage, slots, grad, lr, step_t, weight_decay=0.01,
                beta1=0.9, beta2=0.999, epsilon=1e-8, **_):
    s, g = _adm(storage, slots, grad)
    lr_t = bias_corrected_lr(lr, beta1 ** step_t, beta2 ** step_t)
    step = _adam_step(storage, "adamw", s, g, lr_t, beta1, beta2, epsilon)
    w = storage.values[s]
    storage.values[s] = w - step - lr * weight_decay * w


def apply_ftrl(storage, slots, grad, lr, l1=0.0, l2=0.0,
               lr_power=-0.5, l2_shrinkage=0.0, **_):
    """FTRL-proximal (reference: KvSparseApplyFtrlOp,
    training_ali_ops.cc:431); l2_shrinkage != 0 is the FtrlV2 variant."""
    s, g = _adm(storage, slots, grad)
    n, z = optimizer_slabs(storage, "ftrl", {})
    w = storage.values[s].float()
    n_old = n[s]
    n_new = n_old + g * g
    sigma = (n_new.pow(-lr_power) - n_old.pow(-lr_power)) / lr
    z_new = z[s] + (g + 2.0 * l2_shrinkage * w) - sigma * w
    n[s], z[s] = n_new, z_new
    quad = n_new.pow(-lr_power) / lr + 2.0 * l2
    w_new = torch.where(
        z_new.abs() > l1,
        (torch.sign(z_new) * l1 - z_new) / quad,
        torch.zeros_like(w))
    storage.values[s] = w_new.to(storage.values.dtype)
