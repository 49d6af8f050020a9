"""The sparse optimizer applies of the HIP extension, called directly on raw
tensors: every entry point against ops/sparse_optim_cpu.py (w AND every
state slab, after each of two consecutive applies), the rows no admitted
slot names bit for bit, the rules that share a body bit for bit, the
grid-stride tail past the 65535-block cap, and the launcher's argument
checks. test_gpu_engine.py::test_sparse_apply_matches_cpu covers the way
through hip_backend.sparse_apply and real storages."""
import math
from typing import Callable, NamedTuple, Tuple

import pytest
import torch

from deeprec_amd.ops import sparse_optim_cpu as cpu_apply

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS, M = 1024, 257          # slab rows; unique keys of one apply
DIMS = [1, 3, 8, 20]         # dim 1: M is one thread past a 256-thread block
STEPS = 2                    # the second apply reads state the first wrote
B1, B2, EPS = 0.9, 0.999, 1e-8
TOL = dict(rtol=1e-5, atol=1e-6)  # test_sparse_apply_matches_cpu's

# state slab -> (width or None for dim, initial value)
SLABS = {"adagrad_accum": (None, 0.1), "adagrad_decay_period": (1, 0.0),
         "adam_m": (None, 0.0), "adam_v": (None, 0.0),
         "ftrl_accum": (None, 0.1), "ftrl_linear": (None, 0.0)}


@pytest.fixture(scope="module")
def ext():
    from deeprec_amd.ops.build_ext import require_extension
    return require_extension()


class Store:
    """What sparse_optim_cpu needs of a storage: values, dim, get_slab."""

    def __init__(self, state):
        self.values = state["w"]
        self.dim = self.values.shape[1]
        self.slabs = {k: v for k, v in state.items() if k != "w"}

    def get_slab(self, name, width, init_value, dtype=torch.float32):
        return self.slabs[name]


def lr_t(lr, b1p, b2p):
    return lr * math.sqrt(1 - b2p) / (1 - b1p)


def powers(t):
    """[beta1^t, beta2^t] as the device carries them: fp32."""
    return torch.tensor([B1 ** t, B2 ** t], dtype=torch.float32)


class Case(NamedTuple):
    cpu: str                  # sparse_optim_cpu.apply_<cpu>
    slabs: Tuple[str, ...]    # state slabs, in the entry point's order
    hyper: Callable           # 1-based step -> kwargs of the CPU reference
    gpu: Callable             # (ext, w, slabs, slots, grad, hyper)


def _adam_hyper(t, **kw):
    return dict(lr=0.01, step_t=t, beta1=B1, beta2=B2, epsilon=EPS, **kw)


def _async_hyper(t, beta2=B2, **kw):
    p = powers(t).tolist()  # the same powers, as floats
    return dict(lr=0.01, beta1_power=p[0], beta2_power=p[1], beta1=B1,
                beta2=beta2, epsilon=EPS, **kw)


# RMSProp has no bias correction, so its first step is lr / sqrt(1 - beta2)
# per element and carries the whole error of 1 - beta2. The kernel forms
# 1.0f - beta2 from the fp32 beta2; for 0.999 that is 1.3e-5 off the
# reference's fl32(1 - 0.999), 2.1e-6 in w: outside TOL with the rule
# computed as written (profiles/PERF_LOG.md). 1 - 2^-10 and its complement
# are exact in fp32, which leaves the rule's own arithmetic to compare.
B2_EXACT = 1.0 - 2.0 ** -10


def _decay_hyper(t, rate=0.9, baseline=0.08):
    # cur_period 3 then 4 against pre-set periods {0, 3, 5} (see initial()):
    # dp > 0, dp == 0 and the dp < 0 clamp; 0.1 * 0.9^3 < baseline floors
    return dict(lr=0.1, global_step=2 * t + 4, accumulator_decay_step=2,
                accumulator_decay_rate=rate, accumulator_baseline=baseline,
                epsilon=0.0)


def cur_period(h):
    return float(h["global_step"] // h["accumulator_decay_step"])


def _ftrl_hyper(shrink):
    return lambda t: dict(lr=0.5, l1=0.1, l2=0.01, lr_power=-0.5,
                          l2_shrinkage=shrink)


def _gpu_adam(ext, w, s, sl, g, h):
    ext.apply_adam(w, s[0], s[1], sl, g,
                   lr_t(h["lr"], B1 ** h["step_t"], B2 ** h["step_t"]),
                   h["beta1"], h["beta2"], h["epsilon"])


def _gpu_adamw(ext, w, s, sl, g, h):
    ext.apply_adamw(w, s[0], s[1], sl, g,
                    lr_t(h["lr"], B1 ** h["step_t"], B2 ** h["step_t"]),
                    h["lr"], h["beta1"], h["beta2"], h["epsilon"],
                    h["weight_decay"])


def _gpu_adam_dev(ext, w, s, sl, g, h):
    p = torch.tensor([h["beta1_power"], h["beta2_power"]],
                     dtype=torch.float32, device=DEV)
    ext.apply_adam_dev(w, s[0], s[1], sl, g, h["lr"], h["beta1"], h["beta2"],
                       h["epsilon"], p)


def _gpu_ftrl(ext, w, s, sl, g, h):
    ext.apply_ftrl(w, s[0], s[1], sl, g, h["lr"], h["l1"], h["l2"],
                   h["lr_power"], h["l2_shrinkage"])


CASES = {
    "sgd": Case("sgd", (), lambda t: dict(lr=0.1),
                lambda ext, w, s, sl, g, h: ext.apply_sgd(w, sl, g, h["lr"])),
    "adagrad": Case(
        "adagrad", ("adagrad_accum",), lambda t: dict(lr=0.1, epsilon=0.0),
        lambda ext, w, s, sl, g, h: ext.apply_adagrad(
            w, s[0], sl, g, h["lr"], h["epsilon"])),
    "adagrad_decay": Case(
        "adagrad_decay", ("adagrad_accum", "adagrad_decay_period"),
        _decay_hyper,
        lambda ext, w, s, sl, g, h: ext.apply_adagrad_decay(
            w, s[0], s[1], sl, g, h["lr"], h["epsilon"], cur_period(h),
            h["accumulator_decay_rate"], h["accumulator_baseline"])),
    "adam": Case("adam", ("adam_m", "adam_v"), _adam_hyper, _gpu_adam),
    "adam_dev": Case("adam_async", ("adam_m", "adam_v"), _async_hyper,
                     _gpu_adam_dev),
    "adamw": Case("adamw", ("adam_m", "adam_v"),
                  lambda t: _adam_hyper(t, weight_decay=0.02), _gpu_adamw),
    "rmsprop": Case(
        "adam_async", ("adam_v",),
        lambda t: _async_hyper(t, beta2=B2_EXACT, sparse_rmsprop=True),
        lambda ext, w, s, sl, g, h: ext.apply_rmsprop(
            w, s[0], sl, g, h["lr"], h["beta2"], h["epsilon"])),
    "ftrl": Case("ftrl", ("ftrl_accum", "ftrl_linear"), _ftrl_hyper(0.0),
                 _gpu_ftrl),
    "ftrl_shrinkage": Case("ftrl", ("ftrl_accum", "ftrl_linear"),
                           _ftrl_hyper(0.05), _gpu_ftrl),
}


def inputs(dim):
    """slots [M] int32 (distinct rows, every fifth -1) and STEPS grads."""
    g = torch.Generator().manual_seed(4000 + dim)
    slots = torch.randperm(ROWS, generator=g)[:M].to(torch.int32)
    slots[::5] = -1
    grads = [torch.randn(M, dim, generator=g) for _ in range(STEPS)]
    return slots, grads


def initial(case, dim):
    g = torch.Generator().manual_seed(5000 + dim)
    state = {"w": torch.randn(ROWS, dim, generator=g)}
    for name in case.slabs:
        width, init = SLABS[name]
        state[name] = torch.full((ROWS, width or dim), init)
    if "adagrad_decay_period" in state:
        state["adagrad_decay_period"] = torch.tensor([0.0, 3.0, 5.0])[
            torch.randint(0, 3, (ROWS, 1), generator=g)]
    return state


def _snapshot(state):
    return {k: v.detach().cpu().clone() for k, v in state.items()}


def run_gpu(ext, case, dim):
    """The state after each of the STEPS applies, on the CPU."""
    slots, grads = inputs(dim)
    state = {k: v.to(DEV) for k, v in initial(case, dim).items()}
    slabs = [state[n] for n in case.slabs]
    out = []
    for t, grad in enumerate(grads, 1):
        case.gpu(ext, state["w"], slabs, slots.to(DEV), grad.to(DEV),
                 case.hyper(t))
        out.append(_snapshot(state))
    return out


def run_ref(case, dim):
    slots, grads = inputs(dim)
    state = initial(case, dim)
    out = []
    for t, grad in enumerate(grads, 1):
        getattr(cpu_apply, f"apply_{case.cpu}")(Store(state), slots, grad,
                                                **case.hyper(t))
        out.append(_snapshot(state))
    return out


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32),
                       b.contiguous().view(torch.int32))


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("name", list(CASES))
def test_apply_matches_reference(ext, name, dim):
    case = CASES[name]
    slots, _ = inputs(dim)
    adm = slots[slots >= 0].long()
    rest = torch.ones(ROWS, dtype=torch.bool)
    rest[adm] = False
    before = initial(case, dim)
    got, ref = run_gpu(ext, case, dim), run_ref(case, dim)

    if name == "adagrad_decay":
        dp = cur_period(case.hyper(1)) - before["adagrad_decay_period"][adm]
        assert (dp > 0).any() and (dp == 0).any() and (dp < 0).any()
    if case.cpu == "ftrl":  # both sides of |z| > l1
        w_adm = ref[-1]["w"][adm]
        assert (w_adm == 0).any() and (w_adm != 0).any()

    for t in range(STEPS):
        for k in before:
            torch.testing.assert_close(got[t][k], ref[t][k], **TOL,
                                       msg=lambda s: f"{k} step {t + 1}: {s}")
            # rows no admitted slot names keep their bits
            assert bits_equal(got[t][k][rest], before[k][rest]), (k, t)
        if name == "adagrad_decay":
            period = got[t]["adagrad_decay_period"]
            assert (period[adm] == cur_period(case.hyper(t + 1))).all()


# ---- rules that share a body agree bit for bit ----

@pytest.mark.parametrize("dim", DIMS)
def test_adamw_without_decay_is_adam(ext, dim):
    adamw = CASES["adamw"]._replace(
        hyper=lambda t: _adam_hyper(t, weight_decay=0.0))
    a, b = run_gpu(ext, CASES["adam"], dim), run_gpu(ext, adamw, dim)
    for t in range(STEPS):
        for k in ("w", "adam_m", "adam_v"):
            assert bits_equal(a[t][k], b[t][k]), (k, t)


@pytest.mark.parametrize("dim", DIMS)
def test_adagrad_decay_without_decay_is_adagrad(ext, dim):
    plain = CASES["adagrad_decay"]._replace(
        hyper=lambda t: _decay_hyper(t, rate=1.0, baseline=0.0))
    a, b = run_gpu(ext, CASES["adagrad"], dim), run_gpu(ext, plain, dim)
    for t in range(STEPS):
        for k in ("w", "adagrad_accum"):
            assert bits_equal(a[t][k], b[t][k]), (k, t)


@pytest.mark.parametrize("dim", DIMS)
def test_rmsprop_second_moment_is_adams(ext, dim):
    rmsprop = CASES["rmsprop"]._replace(  # adam's beta2
        hyper=lambda t: _async_hyper(t, sparse_rmsprop=True))
    a, b = run_gpu(ext, CASES["adam"], dim), run_gpu(ext, rmsprop, dim)
    for t in range(STEPS):
        assert bits_equal(a[t]["adam_v"], b[t]["adam_v"]), t


# ---- the one loop: grid-stride tail past the 65535-block cap ----

def test_grid_stride_tail(ext):
    m, dim = 131073, 128  # 16,777,344 elements > 65535 * 256 = 16,776,960
    assert m * dim > 65535 * 256
    g = torch.Generator(device=DEV).manual_seed(7)
    w = torch.randn(m, dim, device=DEV, generator=g)
    grad = torch.randn(m, dim, device=DEV, generator=g)
    # lr = 0.5: lr * g is exact, so fma(-lr, g, w) == w - lr * g bit for bit
    want = w.cpu() - 0.5 * grad.cpu()
    ext.apply_sgd(w, torch.arange(m, dtype=torch.int32, device=DEV), grad,
                  0.5)
    assert bits_equal(w.cpu(), want)


# ---- the launcher refuses what the kernel would index out of bounds ----

def _good(dim=8):
    return dict(w=torch.randn(ROWS, dim, device=DEV),
                accum=torch.full((ROWS, dim), 0.1, device=DEV),
                slots=torch.arange(M, dtype=torch.int32, device=DEV),
                grad=torch.randn(M, dim, device=DEV))


BAD = {
    "int64 slots": lambda a: a.update(slots=a["slots"].long()),
    "cpu slots": lambda a: a.update(slots=a["slots"].cpu()),
    "cpu w": lambda a: a.update(w=a["w"].cpu()),
    "cpu grad": lambda a: a.update(grad=a["grad"].cpu()),
    "short grad": lambda a: a.update(grad=a["grad"][:-1].contiguous()),
    "non-contiguous w": lambda a: a.update(
        w=torch.randn(8, ROWS, device=DEV).t()),
    "transposed slab": lambda a: a.update(
        accum=a["accum"].t().contiguous()),
    "short slab": lambda a: a.update(accum=a["accum"][:-1].contiguous()),
    "fp64 slab": lambda a: a.update(accum=a["accum"].double()),
}


@pytest.mark.parametrize("bad", list(BAD))
def test_launcher_rejects(ext, bad):
    a = _good()
    BAD[bad](a)
    w0 = a["w"].clone()
    with pytest.raises(RuntimeError):
        ext.apply_adagrad(a["w"], a["accum"], a["slots"], a["grad"], 0.1,
                          0.0)
    torch.cuda.synchronize()
    assert torch.equal(a["w"], w0)  # nothing was launched


def test_launcher_rejects_period_and_powers(ext):
    a = _good()
    m, v = torch.zeros_like(a["w"]), torch.zeros_like(a["w"])
    w0 = a["w"].clone()
    with pytest.raises(RuntimeError):  # the period slab is [rows, 1]
        ext.apply_adagrad_decay(a["w"], a["accum"], torch.zeros_like(a["w"]),
                                a["slots"], a["grad"], 0.1, 0.0, 1.0, 0.9,
                                0.0)
    with pytest.raises(RuntimeError):  # powers holds beta1^t and beta2^t
        ext.apply_adam_dev(a["w"], m, v, a["slots"], a["grad"], 0.01, B1, B2,
                           EPS, torch.ones(1, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(a["w"], w0)
