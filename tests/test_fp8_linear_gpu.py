"""Fp8Linear on hardware against the float64 references of
fp8_linear_refs.py: which scale goes with which operand in the three
`_scaled_mm` calls, which saved tensor is transposed, when the fallback
quantizer is taken and when the cached weight codes are refreshed (needs
MI355X). Bounds and cases: fp8_linear_refs.py; their soundness and the
mutants they catch: test_fp8_linear_refs_cpu.py."""
import os

import pytest
import torch
import torch.nn.functional as F

from edge_refs import assert_within
from fp8_linear_refs import (CASES, DY_AMAX, X_AMAX, inputs, make_tensor,
                             ref_codes, reference)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepspeed_amd.ops import fp8_linear as fl
    from deepspeed_amd.ops.fp8_linear import Fp8Linear, _fp8_ok, _quant_hip
    from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"
BF = torch.bfloat16
DTYPES = [torch.bfloat16, torch.float16]
MID = (80, 144, 48)


def _id(v):
    if isinstance(v, tuple):
        return "x".join(map(str, v))
    return str(v).replace("torch.", "")


def _bits(t):
    return t.view(torch.uint8).cpu()


def _layer(c, dtype, with_bias):
    K, N = c["w"].shape[1], c["w"].shape[0]
    lin = Fp8Linear(K, N, bias=with_bias, device=DEV, dtype=dtype)
    with torch.no_grad():
        lin.weight.copy_(c["w"])
        if with_bias:
            lin.bias.copy_(c["bias"])
    return lin


def _count_fallback(monkeypatch):
    """Number of calls of the torch fallback quantizer from here on."""
    calls = []
    real = fl._quant

    def spy(t, dtype, fmax):
        calls.append(tuple(t.shape))
        return real(t, dtype, fmax)
    monkeypatch.setattr(fl, "_quant", spy)
    return calls


def _check(lin, x_leaf, x, dy, r, tol, what):
    """Forward and backward of lin on x (a view of the leaf x_leaf) against
    reference r; returns the outputs."""
    assert _fp8_ok(x, lin.weight)
    y = lin(x)
    assert y.dtype == x.dtype and y.shape == x.shape[:-1] + (r["N"],)
    y.backward(dy)
    got = dict(y=y, dx=x_leaf.grad, dw=lin.weight.grad)
    if lin.bias is not None:
        got["db"] = lin.bias.grad
    assert set(got) == set(tol)
    for name, g in got.items():
        assert g.dtype == x.dtype, name
        assert_within(g, r[name], tol[name], f"{what} {name}")
    return got


# ------------------------------------------ every case, forward + backward
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", CASES, ids=_id)
def test_cases_match_float64_reference(shape, dtype, with_bias, monkeypatch):
    get_ext(required=True)
    c = inputs(shape, dtype)
    r, tol = reference(shape, dtype, with_bias, DEV)
    lin = _layer(c, dtype, with_bias)
    x = c["x"].to(DEV).requires_grad_(True)
    calls = _count_fallback(monkeypatch)
    _check(lin, x, x, c["dy"].to(DEV), r, tol, f"{shape}")
    # bf16 runs the HIP quantizer throughout; fp16 has no kernel, so w, x
    # and dy all take the torch fallback
    assert len(calls) == (0 if dtype == BF else 3), calls
    assert torch.equal(_bits(lin._w8), _bits(r["w8"]))
    assert torch.equal(_bits(lin._wt8), _bits(r["w8"]).t())
    assert torch.equal(lin._sw.cpu(), r["sw"])


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_3d_input(dtype):
    c = inputs(MID, dtype)
    r, tol = reference(MID, dtype, True, DEV)
    lin = _layer(c, dtype, True)
    x = c["x"].to(DEV).reshape(2, 40, 144).requires_grad_(True)
    dy = c["dy"].to(DEV).reshape(2, 40, 48)
    got = _check(lin, x, x, dy, r, tol, "3-d")
    assert got["dx"].shape == (2, 40, 144)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_noncontiguous_x_and_dy(dtype):
    """x and dy are transposed views: the layer must quantize what the view
    holds, and dx must come back in the view's layout."""
    c = inputs(MID, dtype)
    r, tol = reference(MID, dtype, True, DEV)
    lin = _layer(c, dtype, True)
    xt = c["x"].t().contiguous().to(DEV).requires_grad_(True)     # [K, M]
    dy = c["dy"].t().contiguous().to(DEV).t()
    x = xt.t()
    assert not x.is_contiguous() and not dy.is_contiguous()
    assert_within(x, c["x"], 0.0, "view holds the case's x")
    y = lin(x)
    y.backward(dy)
    for name, g in (("y", y), ("dx", xt.grad.t()), ("dw", lin.weight.grad),
                    ("db", lin.bias.grad)):
        assert_within(g, r[name], tol[name], f"strided {name}")


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
def test_x_one_element_off_alignment_takes_fallback(with_bias, monkeypatch):
    """x starts 2 bytes past a 16-byte boundary: _quant_hip takes the torch
    fallback for x (and only for x), with the same result."""
    c = inputs(MID, BF)
    r, tol = reference(MID, BF, with_bias, DEV)
    lin = _layer(c, BF, with_bias)
    M, K, _ = MID
    buf = torch.zeros(M * K + 8, device=DEV, dtype=BF)
    assert buf.data_ptr() % 16 == 0
    x = buf[1:1 + M * K].view(M, K)
    x.copy_(c["x"])
    x = x.detach().requires_grad_(True)
    assert x.data_ptr() % 16 == 2 and x.is_contiguous()
    calls = _count_fallback(monkeypatch)
    _check(lin, x, x, c["dy"].to(DEV), r, tol, "offset x")
    assert calls == [(M, K)], calls


@pytest.mark.parametrize("e5m2", [False, True], ids=["e4m3", "e5m2"])
@pytest.mark.parametrize("shape", [(16, 16), (80, 144), (128, 64)], ids=_id)
def test_quant_hip_arms_bit_identical(shape, e5m2, monkeypatch):
    """The HIP arm (aligned) and the fallback arm (same values one element
    off alignment) return the same codes, transpose and scale."""
    M, K = shape
    g = torch.Generator().manual_seed(M + K)
    src = make_tensor(g, M, K, DY_AMAX if e5m2 else X_AMAX, -1.0, BF)
    a = src.to(DEV)
    buf = torch.zeros(M * K + 8, device=DEV, dtype=BF)
    b = buf[1:1 + M * K].view(M, K)
    b.copy_(a)
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 2
    calls = _count_fallback(monkeypatch)
    a8, at8, sa = _quant_hip(a, e5m2, True)
    assert calls == []
    b8, bt8, sb = _quant_hip(b, e5m2, True)
    assert calls == [(M, K)]
    want, want_scale = ref_codes(a, e5m2)      # on the arms' device
    for got8, gott8, s in ((a8, at8, sa), (b8, bt8, sb)):
        assert got8.dtype == want.dtype and gott8.dtype == want.dtype
        assert s.dtype == torch.float32 and s.dim() == 0
        assert torch.equal(s, want_scale)
        assert torch.equal(_bits(got8), _bits(want))
        assert gott8.shape == (K, M) and gott8.is_contiguous()
        assert torch.equal(_bits(gott8), _bits(want).t())
    # without the transpose the codes are the same ones
    assert torch.equal(_bits(_quant_hip(a, e5m2, False)[0]), _bits(want))
    assert torch.equal(_bits(_quant_hip(b, e5m2, False)[0]), _bits(want))


# ------------------------------------------------------------ all zeros
@pytest.mark.parametrize("arm", ["hip", "fallback", "fp16"])
def test_all_zero_inputs(arm):
    dtype = torch.float16 if arm == "fp16" else BF
    shape = (16, 32, 48)
    M, K, N = shape
    c = inputs(shape, dtype)
    tiny = torch.tensor(1e-12)

    def zeros(rows, cols):
        buf = torch.zeros(rows * cols + 8, device=DEV, dtype=dtype)
        off = 1 if arm == "fallback" else 0
        return buf[off:off + rows * cols].view(rows, cols)

    for e5m2 in (False, True):
        z8, zt8, s = _quant_hip(zeros(M, K), e5m2, True)
        assert torch.equal(s.cpu(), tiny)
        assert (_bits(z8) == 0).all() and (_bits(zt8) == 0).all()

    # x = 0: Y is exactly the bias, dW exactly 0, nothing is NaN
    lin = _layer(c, dtype, True)
    x = zeros(M, K).detach().requires_grad_(True)
    y = lin(x)
    y.backward(c["dy"].to(DEV))
    assert torch.equal(y, lin.bias.detach().expand(M, N))
    assert (lin.weight.grad == 0).all()
    assert torch.isfinite(x.grad).all()
    r, tol = reference(shape, dtype, True, DEV)
    assert_within(x.grad, r["dx"], tol["dx"], "dx at x = 0")

    # dy = 0: every gradient is exactly 0
    lin = _layer(c, dtype, True)
    x = c["x"].to(DEV).requires_grad_(True)
    lin(x).backward(zeros(M, N))
    for name, g in (("dx", x.grad), ("dw", lin.weight.grad),
                    ("db", lin.bias.grad)):
        assert (g == 0).all(), name

    # both 0, no bias: the output is exactly 0 as well
    lin = _layer(c, dtype, False)
    x = zeros(M, K).detach().requires_grad_(True)
    y = lin(x)
    y.backward(zeros(M, N))
    assert (y == 0).all() and (x.grad == 0).all()
    assert (lin.weight.grad == 0).all()


# ----------------------------------------------------------- ineligible
@pytest.mark.parametrize("why", ["M=15", "K=24", "DSAMD_FP8=0"])
def test_ineligible_input_is_plain_linear(why, monkeypatch):
    M, K, N = {"M=15": (15, 32, 48), "K=24": (16, 24, 48),
               "DSAMD_FP8=0": (16, 32, 48)}[why]
    if why == "DSAMD_FP8=0":
        monkeypatch.setenv("DSAMD_FP8", "0")
    else:
        monkeypatch.delenv("DSAMD_FP8", raising=False)
    torch.manual_seed(3)
    lin = Fp8Linear(K, N, bias=True, device=DEV, dtype=BF)
    x = torch.randn(M, K, device=DEV, dtype=BF, requires_grad=True)
    assert _fp8_ok(x, lin.weight) == (why == "DSAMD_FP8=0")
    calls = _count_fallback(monkeypatch)
    y = lin(x)
    assert torch.equal(y, F.linear(x, lin.weight, lin.bias))
    assert calls == [] and lin._w8 is None
    y.backward(torch.randn(M, N, device=DEV, dtype=BF))
    assert calls == [] and lin._w8 is None      # backward is plain too
    assert x.grad is not None and lin.weight.grad is not None


def test_fp8_on_by_default_and_when_set_to_1(monkeypatch):
    c = inputs((16, 16, 16), BF)
    for val in (None, "1"):
        if val is None:
            monkeypatch.delenv("DSAMD_FP8", raising=False)
        else:
            monkeypatch.setenv("DSAMD_FP8", val)
        lin = _layer(c, BF, False)
        lin(c["x"].to(DEV))
        assert lin._w8 is not None


# ---------------------------------------------------------------- cache
def test_cache_reused_until_bump_then_refreshed():
    c = inputs(MID, BF)
    lin = _layer(c, BF, True)
    with torch.no_grad():
        lin.weight.copy_(c["w_prev"])
    x = c["x"].to(DEV)
    lin(x)
    w8, wt8, sw = lin._w8, lin._wt8, lin._sw
    p8, pt8 = w8.data_ptr(), wt8.data_ptr()
    old8, _ = ref_codes(c["w_prev"].to(DEV), False)
    assert torch.equal(_bits(w8), _bits(old8))
    lin(x)
    assert lin._w8 is w8 and lin._wt8 is wt8 and lin._sw is sw
    assert lin._w8.data_ptr() == p8 and lin._wt8.data_ptr() == pt8

    # the optimizer's in-place update; without a bump the cache stands
    # (that is the contract: whoever changes weights bumps the version)
    with torch.no_grad():
        lin.weight.copy_(c["w"])
    lin(x)
    assert lin._w8 is w8 and torch.equal(_bits(lin._w8), _bits(old8))

    fl.bump_fp8_version()
    r, tol = reference(MID, BF, True, DEV)
    assert (_bits(r["w8"]) != _bits(old8)).any()
    xg = x.clone().requires_grad_(True)
    _check(lin, xg, xg, c["dy"].to(DEV), r, tol, "after bump")
    assert lin._w8 is not w8
    assert torch.equal(_bits(lin._w8), _bits(r["w8"]))
    assert torch.equal(_bits(lin._wt8), _bits(r["w8"]).t())
    assert torch.equal(lin._sw.cpu(), r["sw"])
    assert lin._wv == fl._VERSION[0]


def test_two_layers_keep_their_own_cache():
    """The cache is per layer, the version global."""
    c = inputs((16, 32, 48), BF)
    a, b = _layer(c, BF, False), _layer(c, BF, False)
    with torch.no_grad():
        b.weight.copy_(c["w_prev"])
    x = c["x"].to(DEV)
    a(x), b(x)
    for lin, w in ((a, c["w"]), (b, c["w_prev"])):
        assert torch.equal(_bits(lin._w8),
                           _bits(ref_codes(w.to(DEV), False)[0]))
    assert Fp8Linear._w8 is None          # nothing leaked to the class


# --------------------------------------------------------------- engine
class _Wrap(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = Fp8Linear(64, 32, bias=True)

    def forward(self, x, target):
        return F.mse_loss(self.lin(x).float(), target.float())


def test_engine_step_and_checkpoint_load_refresh_cache(tmp_path):
    for k, v in (("RANK", "0"), ("WORLD_SIZE", "1"), ("LOCAL_RANK", "0"),
                 ("MASTER_ADDR", "127.0.0.1"), ("MASTER_PORT", "29519")):
        os.environ.setdefault(k, v)
    import deepspeed_amd
    torch.manual_seed(0)
    with torch.device(DEV):
        model = _Wrap()
    config = {
        "train_micro_batch_size_per_gpu": 16,
        "optimizer": {"type": "AdamW", "params": {"lr": 1e-2}},
        "zero_optimization": {"stage": 1},
        "bf16": {"enabled": True},
    }
    engine, _, _, _ = deepspeed_amd.initialize(model=model, config=config)
    lin = engine.module.lin
    x = torch.randn(16, 64, device=DEV, dtype=BF)
    target = torch.randn(16, 32, device=DEV, dtype=BF)

    def codes_now():
        return ref_codes(lin.weight.detach(), False)

    def step():
        loss = engine(x, target)
        assert lin._wv == fl._VERSION[0]
        want, want_s = codes_now()          # the weight this forward used
        assert torch.equal(_bits(lin._w8), _bits(want))
        assert torch.equal(_bits(lin._wt8), _bits(want).t())
        assert torch.equal(lin._sw, want_s)
        engine.backward(loss)
        v = fl._VERSION[0]
        engine.step()
        assert fl._VERSION[0] > v, "engine.step() did not bump the version"
        return want

    assert lin.weight.dtype == BF
    first = step()
    saved, _ = codes_now()
    assert (_bits(saved) != _bits(first)).any(), "step left the codes alone"
    engine.save_checkpoint(str(tmp_path), tag="t0")
    second = step()                          # asserts the refreshed cache
    assert torch.equal(_bits(second), _bits(saved))
    moved, _ = codes_now()
    assert (_bits(moved) != _bits(saved)).any()
    engine(x, target)                        # cache now holds `moved`
    assert torch.equal(_bits(lin._w8), _bits(moved))

    v = fl._VERSION[0]
    engine.load_checkpoint(str(tmp_path), tag="t0")
    assert fl._VERSION[0] > v, "load_checkpoint did not bump the version"
    engine(x, target)
    want, want_s = codes_now()
    assert torch.equal(_bits(want), _bits(saved)), "checkpoint not restored"
    assert torch.equal(_bits(lin._w8), _bits(saved))
    assert torch.equal(_bits(lin._wt8), _bits(saved).t())
    assert torch.equal(lin._sw, want_s)
    engine.destroy()
