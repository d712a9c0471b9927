"""fp8 amax / cast / cast-transpose HIP kernels: bit-exact against torch's
own float8 casts at tails, misaligned bases, ties, saturation, subnormals,
NaN and inf (needs MI355X). No mismatch allowance anywhere: the kernels
compute x * (1 / max(scale, 1e-12)) in fp32, clamp to the format maximum and
convert with round-to-nearest-even, which is exactly `fp8_codes_ref`."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"
BF = torch.bfloat16
SIZES = [1, 7, 8, 9, 2055, 256 * 8 * 3 + 5]
FORMATS = {False: (torch.float8_e4m3fn, 448.0),
           True: (torch.float8_e5m2, 57344.0)}


def _ext():
    return get_ext(required=True)


def fp8_codes_ref(x, scale, e5m2):
    """uint8 codes of (x.float() * inv).clamp(-fmax, fmax).to(dtype) with
    inv = 1 / max(scale, 1e-12) in fp32. clamp keeps NaN, saturates inf."""
    dt, fmax = FORMATS[e5m2]
    inv = 1.0 / torch.clamp(scale.float().reshape(()), min=1e-12)
    return (x.float() * inv).clamp(-fmax, fmax).to(dt).view(torch.uint8)


def _flat(n, off):
    """As test_kernel_edges_gpu._flat: contiguous [n] bf16 whose base is
    16-byte aligned (off=0) or one element past it (off=1)."""
    buf = (torch.randn(n + 8, device=DEV) * 3.0).to(BF)
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + n]
    assert t.is_contiguous() and t.numel() == n
    return t


# -------------------------------------------------------------------- amax
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_fp8_amax_exact_tail_and_offset(n, off):
    torch.manual_seed(n + off)
    first_tail = (n // 8) * 8 if n % 8 else n - 1
    for pos, val in ((n - 1, -1000.0), (first_tail, 1000.0), (0, -1000.0)):
        x = _flat(n, off)
        x[pos] = val
        got = _ext().fp8_amax(x)
        assert got.shape == (1,) and got.dtype == torch.float32
        assert torch.equal(got[0], x.abs().amax().float()), (n, off, pos)
    x = _flat(n, off)           # no sentinel: plain random data
    assert torch.equal(_ext().fp8_amax(x)[0], x.abs().amax().float())


@pytest.mark.parametrize("n", [1, 9, 2055])
def test_fp8_amax_propagates_nan_and_inf(n):
    """A diverged activation must not get a finite scale."""
    for pos in sorted({0, n - 1, (n // 8) * 8 if n % 8 else n - 1}):
        x = _flat(n, 0)
        x[pos] = float("inf")
        assert _ext().fp8_amax(x)[0].item() == float("inf")
        x[pos] = float("nan")
        assert torch.isnan(_ext().fp8_amax(x)[0]), (n, pos)
        x[pos] = -float("nan")
        assert torch.isnan(_ext().fp8_amax(x)[0]), (n, pos)


# -------------------------------------------------------------------- cast
def _ties(e5m2):
    """Mid-points of adjacent fp8 values, both signs, then the format
    maximum. e4m3: (2m+1)/16 * 2^e, m = 8..15 (as _fp8_ties in
    test_kernel_edges_gpu); e5m2: (2m+1)/8 * 2^e, m = 4..7. Each needs 5
    resp. 4 significant bits, so it is exact in bf16."""
    if e5m2:
        mids = [(2 * m + 1) / 8.0 * 2.0 ** e * s for e in range(-14, 15)
                for m in range(4, 8) for s in (1, -1)]
    else:
        mids = [(2 * m + 1) / 16.0 * 2.0 ** e * s for e in range(-6, 8)
                for m in range(8, 16) for s in (1, -1)]
    return torch.tensor(mids + [FORMATS[e5m2][1]])


def _subnormals(e5m2):
    """Multiples of HALF the smallest fp8 subnormal (2^-9 resp. 2^-16), both
    signs: every second one is a tie between two subnormal codes or 0."""
    step = 2.0 ** (-17 if e5m2 else -10)
    ks = torch.arange(0, 20).float()
    return torch.cat([ks * step, -ks * step])


def _pad8(t):
    return torch.cat([t, torch.zeros((-t.numel()) % 8)])


def _cast_groups(e5m2):
    """(name, bf16 x, fp32 scale). Power-of-two scales make x * inv exact,
    so ties and subnormals reach the converter as exact half-way points."""
    torch.manual_seed(5)
    fmax = FORMATS[e5m2][1]
    rnd = torch.randn(4096) * 3.0
    groups = [
        ("random", rnd, rnd.abs().max() / fmax),
        ("random unit scale", rnd, torch.tensor(1.0)),
        ("saturate", torch.randn(512) * 4.0 * fmax * 0.25, torch.tensor(0.25)),
        ("signed zeros", torch.tensor([0.0, -0.0] * 4), torch.tensor(0.5)),
        ("ties", _pad8(_ties(e5m2)) * 0.125, torch.tensor(0.125)),
        ("fp8 subnormals", _pad8(_subnormals(e5m2)) * 4.0, torch.tensor(4.0)),
        ("bf16 subnormals", _pad8(torch.tensor(
            [2.0 ** -133, -2.0 ** -133, 2.0 ** -126, -2.0 ** -126])),
         torch.tensor(1.0)),
        ("scale below floor", rnd[:64] * 1e-13, torch.tensor(1e-14)),
    ]
    out = []
    for name, x, scale in groups:
        xb = x.to(BF)
        if name in ("ties", "fp8 subnormals"):
            assert torch.equal(xb.float(), x), name     # exact in bf16
        out.append((name, xb.to(DEV), scale.float().reshape(1).to(DEV)))
    return out


@pytest.mark.parametrize("e5m2", [False, True])
def test_fp8_cast_codes_equal_torch(e5m2):
    for name, x, scale in _cast_groups(e5m2):
        ref = fp8_codes_ref(x, scale, e5m2)
        got = _ext().fp8_cast(x, scale, e5m2)
        assert got.dtype == torch.uint8 and got.shape == x.shape
        n_off = int((got != ref).sum())
        assert n_off == 0, f"{name}: {n_off}/{x.numel()} codes differ"
    # saturation really happened, and the tie group really holds ties
    name, x, scale = _cast_groups(e5m2)[2]
    dt, fmax = FORMATS[e5m2]
    assert (fp8_codes_ref(x, scale, e5m2).view(dt).float().abs()
            == fmax).sum() > 50


@pytest.mark.parametrize("e5m2", [False, True])
def test_fp8_cast_nan_and_inf(e5m2):
    """+-inf saturates to +-fmax; NaN becomes the format's NaN."""
    dt, fmax = FORMATS[e5m2]
    x = torch.tensor([float("inf"), -float("inf"), float("nan"),
                      -float("nan"), 1.0, -2.0, 0.0, float("nan")],
                     device=DEV).to(BF)
    scale = torch.ones(1, device=DEV)
    for got in (_ext().fp8_cast(x, scale, e5m2),
                _ext().fp8_cast_transpose(x.view(1, 8), scale, e5m2)[0][0],
                _ext().fp8_cast_transpose(x.view(1, 8), scale, e5m2)[1][:, 0]):
        y = got.view(dt).float().cpu()
        assert y[0] == fmax and y[1] == -fmax
        assert torch.isnan(y[[2, 3, 7]]).all(), y
        assert y[4] == 1.0 and y[5] == -2.0 and y[6] == 0.0
        ref = fp8_codes_ref(x, scale, e5m2).view(dt).float().cpu()
        assert torch.equal(torch.isnan(y), torch.isnan(ref))
        assert torch.equal(y.nan_to_num(), ref.nan_to_num())


# ---------------------------------------------------------- cast-transpose
@pytest.mark.parametrize("e5m2", [False, True])
@pytest.mark.parametrize("M,K", [(1, 8), (64, 64), (65, 72), (63, 136),
                                 (130, 40), (16, 200), (5, 13)])
def test_fp8_cast_transpose_shapes(M, K, e5m2):
    torch.manual_seed(M * 1000 + K)
    fmax = FORMATS[e5m2][1]
    x = (torch.randn(M, K, device=DEV) * 3.0).to(BF)
    x[M - 1, K - 1] = 100.0         # amax at the very last element
    x[0, K - 1] = -50.0             # last column of the first row
    scale = (x.abs().amax().float() / fmax).reshape(1)
    ref = fp8_codes_ref(x, scale, e5m2)
    y, yt = _ext().fp8_cast_transpose(x, scale, e5m2)
    assert y.shape == (M, K) and yt.shape == (K, M)
    assert torch.equal(y, ref)
    assert torch.equal(yt, y.t().contiguous())
    if (M * K) % 8 == 0:
        assert torch.equal(_ext().fp8_cast(x, scale, e5m2), y)


def test_fp8_entry_points_reject_bad_arguments():
    e = _ext()
    x = torch.zeros(8, 16, device=DEV, dtype=BF)
    s = torch.ones(1, device=DEV)
    bad = {
        "amax fp32": lambda: e.fp8_amax(x.float()),
        "amax strided": lambda: e.fp8_amax(x.t()),
        "cast fp32": lambda: e.fp8_cast(x.float(), s, False),
        "cast numel % 8": lambda: e.fp8_cast(x.view(-1)[:13], s, False),
        "cast misaligned": lambda: e.fp8_cast(x.view(-1)[1:9], s, False),
        "cast scale dtype": lambda: e.fp8_cast(x, s.double(), False),
        "cast scale numel": lambda: e.fp8_cast(x, torch.ones(2, device=DEV),
                                               False),
        "cast scale device": lambda: e.fp8_cast(x, s.cpu(), False),
        "ct 3-d": lambda: e.fp8_cast_transpose(x.view(2, 4, 16), s, False),
        "ct strided": lambda: e.fp8_cast_transpose(x.t(), s, False),
        "ct scale device": lambda: e.fp8_cast_transpose(x, s.cpu(), False),
    }
    for name, call in bad.items():
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"'{name}' did not raise")
