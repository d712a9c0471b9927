"""One-pass RMSNorm backward (needs MI355X): dx and the dw partials from a
single read of dy and x, partial rows summed in a fixed order.

Reference: the fp32 formula of `_RMSNormFn.backward`'s CPU branch, fed the
rstd the forward kernel saved. Tolerances: the expressions test_rmsnorm_rows
in test_kernel_edges_gpu.py uses for dx and dw (derived in edge_refs.py),
with their condition terms taken from edge_refs.rmsnorm_ref.
"""
import pytest
import torch

from edge_refs import EPI, U24, assert_within, bf16_tol, rmsnorm_ref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"
BF = torch.bfloat16

# rows: fewer than / more than the fixed grid's workgroups, uneven chunks.
# H: one partly filled vector slot (8, 72), the scalar path (250), the bench
# width (4096, two vectors per thread).
ROWS = [1, 3, 257, 1031]
HS = [8, 72, 250, 4096]
# register-limit arms of the one-pass kernel: three of four vector slots
# (4104), the widest row it takes (8192), the first width past it, which
# takes the two-kernel path (8200); 1031 rows there reach its 16 partial rows
LIMIT_CASES = [(3, 4104), (3, 8192), (3, 8200), (1031, 8200)]


def _ext():
    return get_ext(required=True)


def _inputs(rows, H, offset=0):
    """offset: elements by which every base is shifted off 16-byte alignment."""
    torch.manual_seed(rows * 10007 + H + offset)

    def mk(n, scale, shift=0.0):
        buf = (torch.randn(n + 8, device=DEV) * scale + shift).to(BF)
        assert buf.data_ptr() % 16 == 0
        return buf[offset:offset + n]

    x = mk(rows * H, 1.5).view(rows, H)
    dy = mk(rows * H, 2.0).view(rows, H)
    w = mk(H, 0.7, 1.0)
    if rows:  # sentinels: a dropped last element / last row cannot hide
        x[-1, H - 1] = 1000.0
        dy[-1, H - 1] = 64.0
    return x, w, dy


def _ref_fp32(dy, x, w, rstd):
    """`_RMSNormFn.backward`, CPU branch, verbatim in fp32."""
    H = x.shape[-1]
    x32 = x.float()
    dy32 = dy.float()
    rs = rstd.reshape(*x.shape[:-1], 1).float()
    w32 = w.float()
    g = dy32 * w32
    dot = (g * x32).sum(-1, keepdim=True)
    dx = rs * (g - x32 * dot * rs * rs / H)
    dw = (dy32 * x32 * rs).reshape(-1, H).sum(0)
    return dx, dw


def _check(rows, H, offset=0):
    x, w, dy = _inputs(rows, H, offset)
    if offset:
        assert x.data_ptr() % 16 != 0 and x.is_contiguous()
    y, rstd = _ext().rmsnorm_fwd(x, w, 1e-5)
    dx, dw = _ext().rmsnorm_bwd(dy, x, w, rstd)
    dx2, dw2 = _ext().rmsnorm_bwd(dy, x, w, rstd)
    assert dx.shape == x.shape and dx.dtype == BF
    assert dw.shape == (H,) and dw.dtype == torch.float32
    rdx, rdw = _ref_fp32(dy, x, w, rstd)
    cond = rmsnorm_ref(x, w, dy, 1e-5)
    edx = (dx.double() - rdx.double()).abs().max().item()
    edw = (dw.double() - rdw.double()).abs().max().item()
    print(f"rows {rows} H {H} off {offset}: max|dx err| {edx:.3e} "
          f"max|dw err| {edw:.3e}")
    assert_within(dx, rdx, bf16_tol(rdx.double(), 4 * (H + EPI) * U24 *
                                    cond["dx_terms"]), "dx")
    assert_within(dw, rdw, (rows + H + 2 * EPI) * U24 * cond["dw_abs"], "dw")
    # no atomics: the same call again gives the same bits
    assert torch.equal(dw.view(torch.int32), dw2.view(torch.int32))
    assert torch.equal(dx.view(torch.int16), dx2.view(torch.int16))


@pytest.mark.parametrize("H", HS)
@pytest.mark.parametrize("rows", ROWS)
def test_onepass_rows_by_width(rows, H):
    _check(rows, H)


@pytest.mark.parametrize("rows,H", LIMIT_CASES)
def test_register_limit_and_two_kernel_path(rows, H):
    _check(rows, H)


@pytest.mark.parametrize("rows,H", [(4097, 250), (4097, 8200)])
def test_two_kernel_path_with_64_partial_rows(rows, H):
    # rows > 4096 on the two-kernel path (scalar row / past the register
    # limit): dw partials strided over 64 grid rows
    assert rows > 4096 and (H % 8 or H > 8192)
    _check(rows, H)


@pytest.mark.parametrize("rows,H", [(3073, 64), (3073, 4104)])
def test_onepass_chunks_longer_than_two_rows(rows, H):
    """One-pass kernel (NV = 1 and 4) on chunks of three rows or more, so a
    steady-state row has both a predecessor and a successor in its chunk
    (`more` true on entry and on exit), and a short last chunk."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per = -(-rows // (4 * cus))             # rmsnorm_bwd: 4 workgroups per CU
    assert per >= 3, f"{cus} CUs give chunks of {per} rows: arm not reached"
    assert rows % per, "the last chunk must be shorter than the others"
    assert H % 8 == 0 and H <= 8192
    _check(rows, H)


@pytest.mark.parametrize("rows,H", [(3, 72), (1031, 72)])
def test_unaligned_bases_take_scalar_path(rows, H):
    # a sliced input whose base sits 2 bytes past 16-byte alignment
    _check(rows, H, offset=1)


@pytest.mark.parametrize("H", [8, 250])
def test_zero_rows(H):
    x = torch.empty(0, H, device=DEV, dtype=BF)
    w = torch.ones(H, device=DEV, dtype=BF)
    rstd = torch.empty(0, device=DEV)
    dx, dw = _ext().rmsnorm_bwd(x.clone(), x, w, rstd)
    assert dx.shape == (0, H)
    assert dw.dtype == torch.float32 and torch.equal(
        dw, torch.zeros(H, device=DEV))
