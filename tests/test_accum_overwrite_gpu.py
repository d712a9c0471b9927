"""accum_bf16_to_f32 with the overwrite flag (needs MI355X): dst is written
as float(src) * scale and never read, which the NaN pre-fill proves; without
the flag the kernel accumulates as before."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"
# 1, 7: scalar tail only; 8: vectors only; 1027: vectors + a 3-element tail
SIZES = [1, 7, 8, 1027]


def _views(n, dst_off, src_off, seed):
    """dst/src of n elements starting dst_off/src_off elements into buffers
    whose bases are 16-byte aligned; the elements around them are guards."""
    torch.manual_seed(seed)
    dbuf = torch.full((n + 16,), float("nan"), device=DEV)
    sbuf = (torch.randn(n + 16, device=DEV) * 3.0).to(torch.bfloat16)
    assert dbuf.data_ptr() % 16 == 0 and sbuf.data_ptr() % 16 == 0
    return dbuf, dbuf[dst_off:dst_off + n], sbuf[src_off:src_off + n]


def _bits(t):
    return t.contiguous().view(torch.int32)


# (0, 0) vector path; dst one float off; src one bf16 off; both off
@pytest.mark.parametrize("dst_off,src_off", [(0, 0), (1, 0), (0, 1), (3, 5)])
@pytest.mark.parametrize("scale", [1.0, 0.375])
@pytest.mark.parametrize("n", SIZES)
def test_overwrite_ignores_dst(n, scale, dst_off, src_off):
    ext = get_ext(required=True)
    dbuf, dst, src = _views(n, dst_off, src_off, n)
    ext.accum_bf16_to_f32(dst, src, scale, True)
    want = src.float() * scale
    assert torch.equal(_bits(dst), _bits(want))
    # nothing outside the view was touched
    guard = torch.ones(n + 16, dtype=torch.bool, device=DEV)
    guard[dst_off:dst_off + n] = False
    assert torch.isnan(dbuf[guard]).all()


@pytest.mark.parametrize("dst_off,src_off", [(0, 0), (1, 0), (3, 5)])
@pytest.mark.parametrize("n", SIZES)
def test_default_still_accumulates(n, dst_off, src_off):
    ext = get_ext(required=True)
    dbuf, dst, src = _views(n, dst_off, src_off, n + 1)
    base = torch.randn(n, device=DEV)
    for flag in ((), (False,)):          # default argument and explicit False
        dst.copy_(base)
        ext.accum_bf16_to_f32(dst, src, 0.5, *flag)
        want = base + src.float() * 0.5
        # one fp32 multiply and one add, possibly contracted into one fma
        assert torch.allclose(dst, want, rtol=2.0 ** -23, atol=0.0)
    # overwrite then add is the same as add onto zeros
    ext.accum_bf16_to_f32(dst, src, 1.0, True)
    ext.accum_bf16_to_f32(dst, src, 1.0)
    zero = torch.zeros(n, device=DEV)
    ext.accum_bf16_to_f32(zero, src, 1.0)
    ext.accum_bf16_to_f32(zero, src, 1.0)
    assert torch.equal(_bits(dst), _bits(zero))


def test_empty_and_contract():
    ext = get_ext(required=True)
    ext.accum_bf16_to_f32(torch.empty(0, device=DEV),
                          torch.empty(0, device=DEV, dtype=torch.bfloat16),
                          1.0, True)
    with pytest.raises(RuntimeError):
        ext.accum_bf16_to_f32(torch.empty(4, device=DEV),
                              torch.empty(3, device=DEV,
                                          dtype=torch.bfloat16), 1.0, True)
