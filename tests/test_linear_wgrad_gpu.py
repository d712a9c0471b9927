"""ops/linear.py on hardware (needs MI355X): dw from transposed operands
against the float64 reference and derived bound of linear_wgrad_refs.py; y,
dx and db bit-identical to F.linear's under autograd; and the routing: who
takes the new path and who takes plain F.linear."""
import pytest
import torch
import torch.nn.functional as F

from edge_refs import assert_within
from linear_wgrad_refs import CASES, dw_reference, make_inputs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (transpose dY, transpose X): the three arrangements the table can hold
ARRANGEMENTS = [(True, False), (False, True), (True, True)]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _plain(x, w, b, dy):
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    b = None if b is None else b.detach().clone().requires_grad_(True)
    y = F.linear(x, w, b)
    y.backward(dy)
    return y, x.grad, w.grad, None if b is None else b.grad


def _new(x, w, b, dy, arr):
    from deepspeed_amd.ops.linear import _LinearWgradFn
    x = x.detach().clone().requires_grad_(True)
    w = w.detach().clone().requires_grad_(True)
    b = None if b is None else b.detach().clone().requires_grad_(True)
    y = _LinearWgradFn.apply(x, w, b, *arr)
    y.backward(dy)
    return y, x.grad, w.grad, None if b is None else b.grad


def _check(x, w, b, dy, arr):
    y0, dx0, dw0, db0 = _plain(x, w, b, dy)
    y1, dx1, dw1, db1 = _new(x, w, b, dy, arr)
    assert torch.equal(_bits(y1), _bits(y0))
    assert dx1.shape == x.shape and torch.equal(_bits(dx1), _bits(dx0))
    if b is not None:
        assert torch.equal(_bits(db1), _bits(db0))
    ref, tol = dw_reference(x, dy)
    assert dw1.shape == w.shape and dw1.is_contiguous()
    assert_within(dw1, ref, tol, f"dw {arr}")
    assert_within(dw0, ref, tol, "dw of F.linear")   # the bound is fair


@pytest.mark.parametrize("arr", ARRANGEMENTS)
@pytest.mark.parametrize("T,K,N", CASES)
def test_dw_within_bound_rest_bit_identical(T, K, N, arr):
    x, w, dy = make_inputs(T, K, N, DEV)
    _check(x, w, None, dy, arr)


@pytest.mark.parametrize("arr", ARRANGEMENTS)
def test_three_d_input(arr):
    x, w, dy = make_inputs(130, 72, 40, DEV, lead=(5, 26))
    _check(x, w, None, dy, arr)


@pytest.mark.parametrize("arr", ARRANGEMENTS)
def test_transposed_view_dy(arr):
    x, w, dy = make_inputs(130, 72, 40, DEV)
    dy_t = dy.t().contiguous().t()          # same values, strides (1, T)
    assert not dy_t.is_contiguous()
    _check(x, w, None, dy_t, arr)


@pytest.mark.parametrize("arr", ARRANGEMENTS)
def test_bias(arr):
    x, w, dy = make_inputs(257, 264, 136, DEV)
    b = torch.randn(136, device=DEV).to(torch.bfloat16)
    _check(x, w, b, dy, arr)
    x3, w3, dy3 = make_inputs(130, 72, 40, DEV, lead=(5, 26))
    _check(x3, w3, torch.randn(40, device=DEV).to(torch.bfloat16), dy3, arr)


# ------------------------------------------------------------------ routing
@pytest.fixture
def spy(monkeypatch):
    """Counts the calls of the new Function and lowers the table to a small
    shape, so that eligibility is the only thing a case varies."""
    from deepspeed_amd.ops import linear as L
    calls = []
    real = L._LinearWgradFn.apply

    def counted(*a):
        calls.append(a[3:])
        return real(*a)

    monkeypatch.setattr(L._LinearWgradFn, "apply", staticmethod(counted))
    monkeypatch.setattr(L, "MIN_TOKENS", 64)
    monkeypatch.setattr(L, "WGRAD_ARRANGEMENT", {(40, 72): (True, True)})
    monkeypatch.delenv("DSAMD_WGRAD_TN", raising=False)
    return calls


def _module_step(dtype=torch.bfloat16, T=130, K=72, N=40):
    from deepspeed_amd.ops.linear import WgradLinear
    torch.manual_seed(3)
    lin = torch.nn.Linear(K, N, bias=True, device=DEV, dtype=dtype)
    holder = torch.nn.Sequential(lin)
    assert WgradLinear.convert(holder) == 1 and type(lin) is WgradLinear
    assert list(holder.state_dict()) == ["0.weight", "0.bias"]
    x = torch.randn(T, K, device=DEV, dtype=dtype, requires_grad=True)
    dy = torch.randn(T, N, device=DEV, dtype=dtype)
    lin(x).backward(dy)
    y0, dx0, dw0, db0 = _plain(x, lin.weight, lin.bias, dy)
    return lin, x, dy, dx0, dw0, db0


def test_eligible_module_takes_the_new_path(spy):
    lin, x, dy, dx0, dw0, db0 = _module_step()
    assert spy == [(True, True)]
    assert torch.equal(_bits(x.grad), _bits(dx0))
    assert torch.equal(_bits(lin.bias.grad), _bits(db0))
    ref, tol = dw_reference(x, dy)
    assert_within(lin.weight.grad, ref, tol, "dw through the module")


@pytest.mark.parametrize("why", ["fp16", "T under threshold",
                                 "shape not in table", "no_grad",
                                 "DSAMD_WGRAD_TN=0"])
def test_ineligible_takes_plain_linear(spy, monkeypatch, why):
    kw = {}
    if why == "fp16":
        kw["dtype"] = torch.float16
    elif why == "T under threshold":
        kw["T"] = 63
    elif why == "shape not in table":
        kw["N"] = 48
    elif why == "DSAMD_WGRAD_TN=0":
        monkeypatch.setenv("DSAMD_WGRAD_TN", "0")
    if why == "no_grad":
        from deepspeed_amd.ops.linear import linear
        x, w, _ = make_inputs(130, 72, 40, DEV)
        with torch.no_grad():
            y = linear(x, w.requires_grad_(True))
        assert torch.equal(_bits(y), _bits(F.linear(x, w)))
    else:
        lin, x, dy, dx0, dw0, db0 = _module_step(**kw)
        # plain F.linear: every gradient has the old path's bits
        assert torch.equal(lin.weight.grad, dw0)
        assert torch.equal(x.grad, dx0)
        assert torch.equal(lin.bias.grad, db0)
    assert spy == []


def test_fp8_and_compression_selectors_know_the_class():
    from deepspeed_amd.ops.fp8_linear import Fp8Linear
    from deepspeed_amd.ops.linear import WgradLinear
    m = torch.nn.Sequential(torch.nn.Linear(16, 16), torch.nn.Linear(16, 16))
    assert Fp8Linear.convert(m, include=["0"]) == 1
    assert WgradLinear.convert(m) == 1          # the fp8 layer is left alone
    assert type(m[0]) is Fp8Linear and type(m[1]) is WgradLinear
    assert Fp8Linear.convert(m) == 1            # a re-classed one converts
    assert type(m[1]) is Fp8Linear
