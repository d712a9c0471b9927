"""transpose_bf16 (needs MI355X) equals x.t().contiguous() bit for bit, on
random bf16 bit patterns (NaN and inf payloads included, so everything is
compared as int16), on both sides of the 64 x 64 tile edge, on every
element-by-element arm (K % 8, M % 8, a base one element off alignment)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"
# (257, 1000): K % 8 == 0, M % 8 != 0; (129, 72): one row past two tiles;
# (40, 70): K % 8 != 0 with M % 8 == 0; (2056, 264): several tiles each way,
# every access a 16-byte vector, the last tile of each side partial
SHAPES = [(1, 1), (1, 8), (8, 1), (63, 65), (64, 64), (65, 63), (129, 72),
          (257, 1000), (40, 70), (2056, 264)]
FIRST_ROW, LAST_ROW, FIRST_COL, LAST_COL = 0x1111, 0x2222, 0x3333, 0x4444


def _make(M, K, offset, seed):
    """Random bit patterns in a contiguous [M, K] bf16 view that starts
    `offset` elements into a 16-byte aligned buffer, sentinels on its edge
    rows and columns."""
    g = torch.Generator().manual_seed(seed)
    buf = torch.randint(-2 ** 15, 2 ** 15, (M * K + 8,), generator=g,
                        dtype=torch.int16).to(DEV)
    assert buf.data_ptr() % 16 == 0
    bits = buf[offset:offset + M * K].view(M, K)
    bits[0, :] = FIRST_ROW
    bits[-1, :] = LAST_ROW
    bits[:, 0] = FIRST_COL
    bits[:, -1] = LAST_COL
    return bits.view(torch.bfloat16), bits


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("M,K", SHAPES)
def test_equals_torch_transpose_bitwise(M, K, offset):
    ext = get_ext(required=True)
    x, bits = _make(M, K, offset, seed=M * 1009 + K)
    assert x.is_contiguous() and (x.data_ptr() % 16 == 0) == (offset == 0)
    xt = ext.transpose_bf16(x)
    assert xt.shape == (K, M) and xt.is_contiguous()
    assert xt.dtype == torch.bfloat16
    got = xt.view(torch.int16)
    assert torch.equal(got, bits.t().contiguous())
    # the sentinel rows and columns arrive as the edge columns and rows
    assert (got[-1, :] == LAST_COL).all()
    assert torch.equal(got[0, :], bits[:, 0])
    assert torch.equal(got[:, 0], bits[0, :])
    assert torch.equal(got[:, -1], bits[-1, :])


def test_fp16_is_taken_as_two_byte_elements():
    ext = get_ext(required=True)
    x = torch.randn(65, 72, device=DEV, dtype=torch.float16)
    assert torch.equal(ext.transpose_bf16(x), x.t().contiguous())


def test_non_contiguous_and_wrong_width_are_refused():
    ext = get_ext(required=True)
    x = torch.randn(64, 72, device=DEV, dtype=torch.bfloat16)
    for bad in (x.t(), x[:, :64], x[::2], x.float(), x.reshape(-1),
                x.cpu()):
        with pytest.raises(RuntimeError):
            ext.transpose_bf16(bad)


@pytest.mark.parametrize("M,K", [(0, 8), (8, 0), (0, 0)])
def test_empty(M, K):
    ext = get_ext(required=True)
    xt = ext.transpose_bf16(torch.empty(M, K, device=DEV,
                                        dtype=torch.bfloat16))
    assert xt.shape == (K, M)
    torch.cuda.synchronize()
