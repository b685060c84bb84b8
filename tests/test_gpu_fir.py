"""GPU parity tests for the FIR family (FIRFilter, DecimatingFIRFilter,
PolyPhaseFilterBank, InterpolatingFIRFilter) against the CPU restatement
(oracle/).  EXACT kernels must be bit-identical to the restatement at the
same precision; FMA / FFT kernels within the §8d tolerance against the f64
restatement:  rel_RMS <= 1e-6 and max|err| <= 1e-6 * sum|h| * max|x|."""
import numpy as np
import pytest

import oracle_lib as O
from gpu_util import bits_equal, rel_rms, to_dev, empty_dev, to_host

pytestmark = pytest.mark.gpu

sd = pytest.importorskip("solid_dsp_amd")
from solid_dsp_amd import PolyPhaseFilterBank, InterpolatingFIRFilter  # noqa: E402
from solid_dsp_amd import FIRFilter as _FIRFilter, DecimatingFIRFilter as _DecimatingFIRFilter  # noqa: E402


# The kernel parity tests below run every call as device work (host_step=False): the host
# step for per-sample calls and small host blocks has its own tests (test_host_step_*).
def FIRFilter(*a, **k):
    k.setdefault("host_step", False)
    return _FIRFilter(*a, **k)


def DecimatingFIRFilter(*a, **k):
    k.setdefault("host_step", False)
    return _DecimatingFIRFilter(*a, **k)

C64, C128, F32, F64 = np.complex64, np.complex128, np.float32, np.float64
DTYPES = [  # (sdsp dtype, coef dtype, sample dtype)
    (O.RR32, F32, F32), (O.RC32, F32, C64), (O.CC32, C64, C64),
    (O.RR64, F64, F64), (O.RC64, F64, C128), (O.CC64, C128, C128),
]


def rand(rng, n, dt):
    if np.dtype(dt).kind == "c":
        return (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(dt)
    return rng.standard_normal(n).astype(dt)


# ---------------------------------------------------------------- KATs
def test_fir_kats_through_device():  # src/filter/fir/mod.rs:200-206, 226-232
    f = FIRFilter(np.array([1.0, 2, 3, 4, 5]), 1.0, sample_dtype=C128)
    assert f.execute(2.02 + 0j) == [complex(10.1, 0.0)]
    f = FIRFilter(np.array([1.0, 2, 3, 4, 5]), 1.0, sample_dtype=C128)
    y = f.execute_block(np.array([2.02, 4.04, 1.02, 0.23, 9.19], dtype=C128))
    assert y[4] == complex(60.03, 0.0)


def test_decim_kats_through_device():  # src/filter/fir/decim.rs:213-219, 242-248
    d = DecimatingFIRFilter(np.array([1.0, 2, 3, 4, 5]), 1.0, 2, sample_dtype=C128)
    assert d.execute(2.02 + 0j) == []
    assert d.execute(4.04 + 0j) == [complex(28.28, 0.0)]
    d = DecimatingFIRFilter(np.array([1.0, 2, 3, 4, 5]), 1.0, 2, sample_dtype=C128)
    y = d.execute_block(np.array([2.02, 4.04, 1.02, 0.23], dtype=C128))
    assert list(y) == [complex(28.28, 0.0), complex(21.39, 0.0)]


def test_accessors_mirror_reference():
    f = FIRFilter(np.arange(1.0, 6.0), 1.0, sample_dtype=C128)
    f.set_scale(2.0)
    assert f.get_scale() == 2.0  # fir/mod.rs:103-124
    assert f.len() == 5 and not f.is_empty()
    assert list(f.coefficients()) == [5.0, 4.0, 3.0, 2.0, 1.0]  # REVERSE storage
    d = DecimatingFIRFilter(np.zeros(12), 1.0, 2, sample_dtype=C128)
    assert d.get_decimation() == 2 and d.len() == 12


def test_errors_mirror_reference():
    with pytest.raises(sd.SdspError) as e:
        FIRFilter(np.array([], dtype=F64), 1.0)
    assert e.value.code == 1
    with pytest.raises(sd.SdspError) as e:
        DecimatingFIRFilter(np.ones(3), 1.0, 0)
    assert e.value.code == 2
    with pytest.raises(sd.SdspError) as e:
        InterpolatingFIRFilter(np.ones(3), 0)
    assert e.value.code == 3
    with pytest.raises(sd.SdspError) as e:
        PolyPhaseFilterBank(np.ones(3), 0, 1.0)
    assert e.value.code == 4


def test_freq_response_and_group_delay_match_oracle():  # fir/mod.rs:253-261, 284-291
    h = O.firdes_notch(25, 0.35, 120.0)
    f = FIRFilter(h, 1.0, sample_dtype=F64)
    r = f.frequency_response(0.0)
    assert round(r.real) == 1.0 and r.imag == 0.0
    o = O.fir(O.RR64, h, 1.0)
    for fr in (0.0, 0.1, -0.3, 0.5):
        assert f.frequency_response(fr) == o.frequency_response(fr)
        assert f.group_delay(fr) == o.group_delay(fr)
    h12 = O.firdes_notch(12, 0.35, 120.0)
    assert int(FIRFilter(h12, 1.0, sample_dtype=F64).group_delay(0.0) + 0.5) == 12


# ---------------------------------------------------------------- exact FIR parity
@pytest.mark.parametrize("dt,cdt,sdt", DTYPES)
@pytest.mark.parametrize("L", [1, 5, 63, 256, 300, 777])
def test_fir_exact_bit_parity(dt, cdt, sdt, L):
    rng = np.random.default_rng(L * 7 + dt)
    h = rand(rng, L, cdt)
    scale = cdt(0.75) if np.dtype(cdt).kind == "f" else cdt(0.75 - 0.25j)
    x = rand(rng, 5000, sdt)
    f = FIRFilter(h, scale, sample_dtype=sdt, algo=sd.ALGO_EXACT)
    o = O.fir(dt, h, scale)
    # streaming across calls of ragged sizes, including empty and single-sample blocks
    cuts = [0, 1, 1, 37, 37, 2048, 4999, 5000]
    for a, b in zip(cuts[:-1], cuts[1:]):
        y = f.execute_block(x[a:b])
        yo = o.execute_block(x[a:b])
        assert bits_equal(y, yo), (L, a, b)


FMA_LS = [1, 5, 255, 256, 257, 777]  # either side of the 256-tap LDS chunk; partial last tap groups for R = 4 and 8
# the ragged cuts of test_fir_exact_bit_parity, then a call of more than two tiles of the widest
# type (2 * 256 * 8 outputs)
FMA_CUTS = [0, 1, 1, 37, 37, 2048, 4999, 5000, 9500]


def _fma_inputs(dt, cdt, sdt, L, n):
    rng = np.random.default_rng(L * 7 + dt)
    h = rand(rng, L, cdt)
    scale = cdt(0.75) if np.dtype(cdt).kind == "f" else cdt(0.75 - 0.25j)
    return h, scale, rand(rng, n, sdt)


def _fma_refs(dt, cdt, sdt, h, scale, x, what):
    """the f64 restatement, after asserting that the reference-order loop at the handle's own
    precision meets the tolerance on these inputs (so a fused kernel that misses it is wrong, not
    unlucky: on the CPU it reaches at most 5.1e-7 rel-RMS, at L = 777 with complex taps, and at most
    0.10 of the max bound, at L = 1)"""
    wc = C128 if np.dtype(cdt).kind == "c" else F64
    ws = C128 if np.dtype(sdt).kind == "c" else F64
    tol = 1e-6 if dt <= O.CC32 else 1e-13
    ref = O.fir(_wide(dt), h.astype(wc), wc(scale)).execute_block(x.astype(ws))
    own = O.fir(dt, h, scale).execute_block(x)
    print(f"{what}: reference order at own precision rel-RMS {rel_rms(own, ref):.3e}")
    assert_fir_tol(own, ref, h * scale, x, tol)
    return ref, tol


@pytest.mark.parametrize("dt,cdt,sdt", DTYPES)
def test_fir_fma_tolerance(dt, cdt, sdt):
    """fir_direct_kernel<..., false> on every type pair, L on either side of the 256-tap LDS chunk
    and with partial last tap groups, streamed over ragged calls (empty, one sample, a call of more
    than two tiles): both section-8d criteria against the f64 restatement, 1e-6 for 32-bit samples
    and 1e-13 for 64-bit (an f64 kernel that computed in f32 would miss it by six orders).
    Measured on MI355X (profiles/r16/LAB.md P3): at most 7.0e-7 (CC32, L = 777), 1.6e-15 (CC64)"""
    rng = np.random.default_rng(11)
    h = rand(rng, 256, cdt)
    x = rand(rng, 20000, sdt)
    y = FIRFilter(h, 1.0, sample_dtype=sdt, algo=sd.ALGO_FMA).execute_block(x)
    ref = O.fir(O.CC64, h.astype(C128), 1.0 + 0j).execute_block(x.astype(C128))
    assert_fir_tol(y, ref, h, x, 1e-6 if dt <= O.CC32 else 1e-13)
    for L in FMA_LS:
        h, scale, x = _fma_inputs(dt, cdt, sdt, L, FMA_CUTS[-1])
        ref, tol = _fma_refs(dt, cdt, sdt, h, scale, x, f"dtype {dt} L={L}")
        f = FIRFilter(h, scale, sample_dtype=sdt, algo=sd.ALGO_FMA)
        y = np.concatenate([f.execute_block(x[a:b]) for a, b in zip(FMA_CUTS[:-1], FMA_CUTS[1:])])
        print(f"dtype {dt} L={L}: fused kernel rel-RMS {rel_rms(y, ref):.3e}")
        assert_fir_tol(y, ref, h * scale, x, tol)
        if L > 1:
            assert bits_equal(f.get_state()[0], x[-(L - 1):])


@pytest.mark.parametrize("dt,cdt,sdt", DTYPES)
def test_fir_fma_three_channels_device(dt, cdt, sdt):
    """three channels on device buffers, two calls (the second reads each channel's own history),
    L = 257 (a second LDS chunk of one tap), every channel under both criteria"""
    import torch
    L, ch, n1, n2 = 257, 3, 4099, 2500
    h, scale, x = _fma_inputs(dt, cdt, sdt, L, ch * (n1 + n2))
    x = x.reshape(ch, n1 + n2)
    f = FIRFilter(h, scale, sample_dtype=sdt, channels=ch, algo=sd.ALGO_FMA)
    ys = []
    for a, b in ((0, n1), (n1, n1 + n2)):
        d_in = to_dev(x[:, a:b].reshape(-1))
        d_out = empty_dev(ch * (b - a), sdt)
        assert f.execute_block_device(d_in, b - a, d_out, torch.cuda.current_stream()) == b - a
        ys.append(to_host(d_out).reshape(ch, b - a))
    y = np.concatenate(ys, axis=1)
    for c in range(ch):
        ref, tol = _fma_refs(dt, cdt, sdt, h, scale, x[c], f"dtype {dt} channel {c}")
        assert_fir_tol(y[c], ref, h * scale, x[c], tol)


def _f32_taps(L, fc):
    return O.firdes_kaiser(L, fc, 80.0, 0.0).astype(F32)


@pytest.mark.parametrize("dt,cdt", [(O.RC32, F32), (O.CC32, C64)])
@pytest.mark.parametrize("L", [2, 64, 256, 257, 1000])
def test_fir_fft_tolerance(dt, cdt, L):
    # overlap-save vs the f64 restatement on the same f32-representable operands (§8d)
    h = _f32_taps(L, 0.1)
    if cdt == C64:
        h = (h * np.exp(2j * np.pi * 0.05 * np.arange(L))).astype(C64)
    x = O.synth(20250226, 0, 0, 300000, complex_=True)
    f = FIRFilter(h, cdt(0.2), sample_dtype=C64, algo=sd.ALGO_FFT)
    y = np.concatenate([f.execute_block(x[:70001]), f.execute_block(x[70001:])])
    ref = O.fir(O.CC64, h.astype(C128), 0.2 + 0j).execute_block(x.astype(C128))
    assert rel_rms(y, ref) <= 1e-6
    bound = 1e-6 * np.abs(h).sum() * 0.2 * np.abs(x).max()
    assert np.abs(y - ref).max() <= bound


OLS_ONESHOT, OLS_PERSISTENT, OLS_SCALAR, OLS_ONESHOT_WIDE = 0, 1, 2, 3
TUNE_OLS_KERNEL = 14


@pytest.mark.parametrize("L", [2, 64, 256, 257, 700, 1025, 2000, 3841])
@pytest.mark.parametrize("ch", [1, 2, 3])
@pytest.mark.parametrize("kern", [OLS_ONESHOT, OLS_ONESHOT_WIDE])
def test_fir_fft_oneshot_kernel_tolerance(L, ch, kern):
    # default kernel (one-shot, XCD-ordered, every segment of the call in one grid: the first
    # segments read the history, the last one is bounded by the stream and writes the next
    # history), ragged calls that cover single-segment calls (n < one window), calls shorter
    # than the history (n = 1: the separate history update), history carry and both edges,
    # every halo size h2 = 1..15; ch = 3 with odd n falls back to the scalar kernel (8-byte
    # rows).  kern = 3: the same kernel with 16-byte lanes
    h = _f32_taps(L, 0.1)
    h = (h * np.exp(2j * np.pi * 0.05 * np.arange(L))).astype(C64)
    x = O.synth(20250229, 6, 0, 300000 * ch, complex_=True).reshape(ch, -1) if ch > 1 else \
        O.synth(20250229, 6, 0, 300000, complex_=True)
    f = FIRFilter(h, C64(0.2), sample_dtype=C64, channels=ch, algo=sd.ALGO_FFT)
    assert sd.lib().sdsp_fir_set_tuning(f._h, TUNE_OLS_KERNEL, kern) == 0
    cuts = [0, 1, 3000, 7001, 70002, 207714, 207715, 300000]
    y = np.concatenate([f.execute_block(x[..., a:b]) for a, b in zip(cuts[:-1], cuts[1:])], axis=-1)
    hist, _ = f.get_state()
    assert bits_equal(hist, x[..., -(L - 1):].reshape(-1))
    for c in range(ch):
        xc = x[c] if ch > 1 else x
        yc = y[c] if ch > 1 else y
        ref = O.fir(O.CC64, h.astype(C128), 0.2 + 0j).execute_block(xc.astype(C128))
        assert rel_rms(yc, ref) <= 1e-6, (L, ch, c)
        bound = 1e-6 * np.abs(h).sum() * 0.2 * np.abs(xc).max()
        assert np.abs(yc - ref).max() <= bound, (L, ch, c)


@pytest.mark.parametrize("L", [256, 700])
def test_fir_fft_blocks_of_whole_segments(L):
    """blocks whose last segment window ends exactly at the block end (n a multiple of the
    segment advance V = 4096 - 256 h2): that segment still runs in the boundary launch, which
    writes the next call's history -- three such blocks, then a ragged one"""
    h = _f32_taps(L, 0.1)
    h = (h * np.exp(2j * np.pi * 0.05 * np.arange(L))).astype(C64)
    V = 4096 - 256 * (-(-(L - 1) // 256))
    x = O.synth(20250230, 2, 0, 3 * 20 * V + 1234, complex_=True)
    f = FIRFilter(h, C64(0.2), sample_dtype=C64, algo=sd.ALGO_FFT)
    cuts = [0, 20 * V, 40 * V, 60 * V, len(x)]
    y = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        y.append(f.execute_block(x[a:b]))
        hist, _ = f.get_state()
        assert bits_equal(hist, x[b - (L - 1):b]), (a, b)
    y = np.concatenate(y)
    ref = O.fir(O.CC64, h.astype(C128), 0.2 + 0j).execute_block(x.astype(C128))
    assert rel_rms(y, ref) <= 1e-6
    assert np.abs(y - ref).max() <= 1e-6 * np.abs(h).sum() * 0.2 * np.abs(x).max()


@pytest.mark.parametrize("L", [2, 64, 257, 513, 1025])
@pytest.mark.parametrize("ch", [1, 3])
def test_fir_fft_persistent_kernel_bit_identical(L, ch):
    # persistent packed interior kernel (SDSP_TUNE_OLS_KERNEL = 1) + boundary kernel vs the
    # scalar overlap-save kernel (= 2): the same IEEE operations per component, so identical bits
    h = _f32_taps(L, 0.1)
    h = (h * np.exp(2j * np.pi * 0.05 * np.arange(L))).astype(C64)
    x = O.synth(20250227, 4, 0, 300000 * ch, complex_=True).reshape(ch, -1) if ch > 1 else \
        O.synth(20250227, 4, 0, 300000, complex_=True)
    a = FIRFilter(h, C64(0.2), sample_dtype=C64, channels=ch, algo=sd.ALGO_FFT)
    b = FIRFilter(h, C64(0.2), sample_dtype=C64, channels=ch, algo=sd.ALGO_FFT)
    assert sd.lib().sdsp_fir_set_tuning(a._h, TUNE_OLS_KERNEL, OLS_PERSISTENT) == 0
    assert sd.lib().sdsp_fir_set_tuning(b._h, TUNE_OLS_KERNEL, OLS_SCALAR) == 0
    cuts = [0, 1, 3000, 7002, 70002, 207714, 300000]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        xa = x[..., lo:hi]
        assert bits_equal(a.execute_block(xa), b.execute_block(xa)), (L, ch, lo, hi)


def test_fir_tuning_rejects_retired_and_bad_keys():
    # no tuning value may leave the output unwritten: retired ablation keys are refused
    f = FIRFilter(_f32_taps(64, 0.1), F32(0.2), sample_dtype=C64, algo=sd.ALGO_FFT)
    for key in (1, 2, 3, 4, 5, 10, 11, 12, 13, 99):
        assert sd.lib().sdsp_fir_set_tuning(f._h, key, 1) == 90, key
    assert sd.lib().sdsp_fir_set_tuning(f._h, TUNE_OLS_KERNEL, 4) == 90
    for v in (OLS_ONESHOT, OLS_PERSISTENT, OLS_SCALAR, OLS_ONESHOT_WIDE):
        assert sd.lib().sdsp_fir_set_tuning(f._h, TUNE_OLS_KERNEL, v) == 0


def test_fir_default_algo_is_exact_for_large_blocks():
    # a handle built with no algo is bit-identical to the reference restatement at any block
    # size (the overlap-save and scan kernels are opt-in)
    h = _f32_taps(256, 0.1)
    x = O.synth(11, 1, 0, 1 << 17, complex_=True)
    f = FIRFilter(h, F32(0.2), sample_dtype=C64)
    assert bits_equal(f.execute_block(x), O.fir(O.RC32, h, F32(0.2)).execute_block(x))


def test_fir_rejects_in_place_and_bad_device_buffers():
    import torch
    h = _f32_taps(64, 0.1)
    n = 1 << 16
    f = FIRFilter(h, F32(0.2), sample_dtype=C64, algo=sd.ALGO_FFT)
    buf = to_dev(O.synth(3, 0, 0, 2 * n, complex_=True))
    with pytest.raises(sd.SdspError) as e:  # in place
        f.execute_block_device(buf, n, buf)
    assert e.value.code == 90
    with pytest.raises(sd.SdspError):  # partial overlap
        f.execute_block_device(buf, n, buf[n // 2:])
    ok = empty_dev(n, C64)
    with pytest.raises(ValueError):  # undersized output
        f.execute_block_device(buf[:n], n, ok[: n - 1])
    with pytest.raises(ValueError):  # wrong dtype
        f.execute_block_device(buf[:n].view(torch.float32), n, ok)
    with pytest.raises(ValueError):  # host tensor
        f.execute_block_device(torch.zeros(n, dtype=torch.complex64), n, ok)
    assert f.execute_block_device(buf[:n], n, ok) == n


def test_fir_side_stream_set_scale_and_state_are_ordered():
    # work queued on a caller stream must finish before set_scale's table rebuild,
    # get_state, clone or reset touch the handle's device buffers
    import torch
    h = _f32_taps(256, 0.1)
    n = 1 << 22
    x = O.synth(5, 2, 0, n, complex_=True)
    d_in = to_dev(x)
    s = torch.cuda.Stream()
    f = FIRFilter(h, F32(0.2), sample_dtype=C64, algo=sd.ALGO_FFT)
    outs = [empty_dev(n, C64) for _ in range(2)]
    with torch.cuda.stream(s):
        f.execute_block_device(d_in, n, outs[0], s)
        f.set_scale(F32(0.5))
        f.execute_block_device(d_in, n, outs[1], s)
        hist, _ = f.get_state()
        g = f.clone()
    torch.cuda.synchronize()
    assert bits_equal(hist, x[-255:])
    ref = FIRFilter(h, F32(0.2), sample_dtype=C64, algo=sd.ALGO_FFT)
    r0 = ref.execute_block(x)
    ref.set_scale(F32(0.5))
    r1 = ref.execute_block(x)
    assert bits_equal(to_host(outs[0]), r0) and bits_equal(to_host(outs[1]), r1)
    assert bits_equal(g.execute_block(x[:1000]), ref.execute_block(x[:1000]))


def test_fir_fft_matches_exact_kernel_across_calls():
    h = _f32_taps(256, 0.1)
    x = O.synth(7, 3, 0, 200000, complex_=True)
    a = FIRFilter(h, F32(0.2), sample_dtype=C64, algo=sd.ALGO_FFT)
    b = FIRFilter(h, F32(0.2), sample_dtype=C64, algo=sd.ALGO_EXACT)
    ya = np.concatenate([a.execute_block(x[i:i + 65537]) for i in range(0, len(x), 65537)])
    yb = b.execute_block(x)
    assert rel_rms(ya, yb) <= 1e-6


def test_fir_state_clone_reset():
    rng = np.random.default_rng(5)
    h = rand(rng, 31, F64)
    x = rand(rng, 400, C128)
    f = FIRFilter(h, 1.0, sample_dtype=C128, algo=sd.ALGO_EXACT)
    f.execute_block(x[:200])
    g = f.clone()
    assert bits_equal(f.execute_block(x[200:]), g.execute_block(x[200:]))
    hist, ph = g.get_state()
    assert bits_equal(hist, x[-30:])
    f.reset()
    assert bits_equal(f.execute_block(x[:50]), O.fir(O.RC64, h, 1.0).execute_block(x[:50]))
    # clone of a decimating handle, 3 channels, at a non-zero phase (7 inputs, M = 3: phase 1)
    h9 = rand(rng, 9, F64)
    x3 = rand(rng, 3 * 18, C128).reshape(3, 18)
    d = DecimatingFIRFilter(h9, 0.5, 3, sample_dtype=C128, channels=3, algo=sd.ALGO_EXACT)
    d.execute_block(x3[:, :7])
    c = d.clone()
    hist, ph = c.get_state()
    assert ph == 1 and d.get_state()[1] == 1
    assert bits_equal(hist.reshape(3, 8)[:, 1:], x3[:, :7]) and not hist.reshape(3, 8)[:, 0].any()
    yc = c.execute_block(x3[:, 7:])
    assert yc.shape == (3, 4)
    assert bits_equal(d.execute_block(x3[:, 7:]), yc)
    for ch in range(3):
        o = O.decim(O.RC64, h9, 0.5, 3)
        o.execute_block(x3[ch, :7])
        assert bits_equal(yc[ch], o.execute_block(x3[ch, 7:]))


def test_fir_multichannel_device_matches_single():
    import torch
    rng = np.random.default_rng(9)
    h = _f32_taps(256, 0.1)
    ch, n = 3, 100000
    x = np.stack([O.synth(1, c, 0, n, complex_=True) for c in range(ch)])
    f = FIRFilter(h, F32(0.2), sample_dtype=C64, channels=ch, algo=sd.ALGO_EXACT)
    d_in = to_dev(x.reshape(-1))
    d_out = empty_dev(ch * n, C64)
    f.execute_block_device(d_in, n, d_out, torch.cuda.current_stream())
    y = to_host(d_out).reshape(ch, n)
    for c in range(ch):
        ref = O.fir(O.RC32, h, F32(0.2)).execute_block(x[c])
        assert bits_equal(y[c], ref)


# ---------------------------------------------------------------- decimator
@pytest.mark.parametrize("dt,cdt,sdt", DTYPES)
@pytest.mark.parametrize("L,M", [(5, 2), (256, 32), (300, 7), (16, 64), (1, 3)])
def test_decim_exact_bit_parity(dt, cdt, sdt, L, M):
    rng = np.random.default_rng(L + M + dt)
    h = rand(rng, L, cdt)
    x = rand(rng, 3000, sdt)
    d = DecimatingFIRFilter(h, cdt(0.5), M, sample_dtype=sdt, algo=sd.ALGO_EXACT)
    o = O.decim(dt, h, cdt(0.5), M)
    for a, b in [(0, 1), (1, 2), (2, 35), (35, 35), (35, 1700), (1700, 3000)]:
        y = d.execute_block(x[a:b])
        yo = o.execute_block(x[a:b])
        assert bits_equal(y, yo), (a, b)
    d.push(x[0]); o.push(x[0])
    d.write(x[:13]); o.write(x[:13])
    assert bits_equal(d.execute_block(x[:500]), o.execute_block(x[:500]))


def _wide(dt):
    return {O.RR32: O.RR64, O.RC32: O.RC64, O.CC32: O.CC64}.get(dt, dt)


def assert_fir_tol(y, ref, h, x, tol):
    """§8d, both criteria: rel_RMS <= tol and max|err| <= tol * sum|h| * max|x|"""
    y = np.asarray(y, dtype=np.complex128)
    ref = np.asarray(ref, dtype=np.complex128)
    assert y.shape == ref.shape
    assert rel_rms(y, ref) <= tol, rel_rms(y, ref)
    bound = tol * float(np.sum(np.abs(np.asarray(h, dtype=np.complex128)))) * \
        float(np.max(np.abs(np.asarray(x, dtype=np.complex128))))
    err = float(np.max(np.abs(y - ref))) if y.size else 0.0
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("dt,cdt,sdt", DTYPES)
@pytest.mark.parametrize("L,M", [(256, 32), (128, 16), (64, 8), (512, 64), (32, 16), (1024, 64), (300, 7)])
def test_decim_fma_tolerance(dt, cdt, sdt, L, M):
    # column-parallel polyphase kernel (L = K*M, K in {2,4,8,16}) or the tiled fallback;
    # streaming over ragged calls with push/write phase moves, vs the f64 restatement
    rng = np.random.default_rng(L * 3 + M + dt)
    h = rand(rng, L, cdt)
    x = rand(rng, 200000, sdt)
    d = DecimatingFIRFilter(h, cdt(0.5), M, sample_dtype=sdt, algo=sd.ALGO_FMA)
    w = _wide(dt)
    wide = {O.RR64: F64, O.RC64: F64, O.CC64: C128}[w]
    o = O.decim(w, h.astype(wide), wide(0.5), M)
    xw = x.astype(C128 if np.dtype(sdt).kind == "c" else F64)
    tol = 1e-6 if np.dtype(sdt).itemsize <= 8 and sdt != F64 else 1e-13
    ys, yos = [], []
    for a, b in [(0, 1), (1, 2), (2, 35), (35, 35), (35, 17000), (17000, 150001), (150001, 200000)]:
        ys.append(d.execute_block(x[a:b]))
        yos.append(o.execute_block(xw[a:b]))
    assert_fir_tol(np.concatenate(ys), np.concatenate(yos), h * 0.5, x, tol)
    d.push(x[0]); o.push(xw[0])
    d.write(x[:13]); o.write(xw[:13])
    assert_fir_tol(d.execute_block(x[:50000]), o.execute_block(xw[:50000]), h * 0.5, x, tol)


def test_decim_fma_multichannel_device():
    import torch
    h = O.firdes_kaiser(256, 1.0 / 64, 80.0, 0.0).astype(F32)
    ch, n = 3, 1 << 20
    x = np.stack([O.synth(2, c, 0, n, complex_=True) for c in range(ch)])
    d = DecimatingFIRFilter(h, F32(1.0 / 32), 32, sample_dtype=C64, channels=ch, algo=sd.ALGO_FMA)
    d_in = to_dev(x.reshape(-1))
    d_out = empty_dev(ch * (n // 32), C64)
    assert d.execute_block_device(d_in, n, d_out, torch.cuda.current_stream()) == n // 32
    y = to_host(d_out).reshape(ch, n // 32)
    for c in range(ch):
        ref = O.decim(O.RC64, h.astype(F64), 1.0 / 32, 32).execute_block(x[c].astype(C128))
        assert_fir_tol(y[c], ref, h / 32, x[c], 1e-6)


def test_decim_cfg4_fma_ragged_phase_moves():
    """the cfg4 shape (firdes_kaiser(256, 1/64), M = 32, crcf) on the FMA
    polyphase kernel over ragged calls with push/write phase moves, both §8d criteria
    (decim.rs:115-139, 221-256)"""
    import torch
    h = O.firdes_kaiser(256, 1.0 / 64, 80.0, 0.0).astype(F32)
    x = O.synth(20250226, 4, 0, 1 << 20, complex_=True)
    d = DecimatingFIRFilter(h, F32(1.0 / 32), 32, sample_dtype=C64, algo=sd.ALGO_FMA)
    o = O.decim(O.RC64, h.astype(F64), 1.0 / 32, 32)
    xw = x.astype(C128)
    ys, yos = [], []
    i = 0
    for k, op in [(1, "b"), (31, "b"), (5, "w"), (1, "p"), (100000, "b"), (7, "p"), (17, "w"), (333333, "d"),
                  (1, "b"), (64, "b"), (3, "w"), (200000, "d"), (1000, "b")]:
        seg, segw = x[i:i + k], xw[i:i + k]
        if op == "b":
            ys.append(d.execute_block(seg))
            yos.append(o.execute_block(segw))
        elif op == "d":
            d_in = to_dev(seg)
            d_out = empty_dev(max(d.output_count(k), 1), C64)
            nout = d.execute_block_device(d_in, k, d_out, torch.cuda.current_stream())
            ys.append(to_host(d_out)[:nout])
            yos.append(o.execute_block(segw))
        elif op == "w":
            d.write(seg); o.write(segw)
        else:
            for v, vw in zip(seg, segw):
                d.push(v); o.push(vw)
        i += k
    y, yo = np.concatenate(ys), np.concatenate(yos)
    assert len(y) > 19000
    assert_fir_tol(y, yo, h / 32, x[:i], 1e-6)


def test_decim_cfg4_shape():
    # cfg4: 32 branches x 8 taps, M = 32, crcf
    h = O.firdes_kaiser(256, 1.0 / 64, 80.0, 0.0).astype(F32)
    x = O.synth(20250226, 4, 0, 1 << 18, complex_=True)
    d = DecimatingFIRFilter(h, F32(1.0 / 32), 32, sample_dtype=C64, algo=sd.ALGO_EXACT)
    y = d.execute_block(x)
    assert len(y) == (1 << 18) // 32
    assert bits_equal(y, O.decim(O.RC32, h, F32(1.0 / 32), 32).execute_block(x))
    ref = O.decim(O.RC64, h.astype(F64), 1.0 / 32, 32).execute_block(x.astype(C128))
    assert rel_rms(y, ref) <= 1e-6


# ---------------------------------------------------------------- PFB / interpolator
@pytest.mark.parametrize("dt,cdt,sdt", DTYPES)
@pytest.mark.parametrize("L,M", [(18, 4), (64, 8), (10, 4), (7, 7)])
def test_pfb_exact_bit_parity(dt, cdt, sdt, L, M):
    rng = np.random.default_rng(L * M + dt)
    h = rand(rng, L, cdt)
    x = rand(rng, 700, sdt)
    p = PolyPhaseFilterBank(h, M, cdt(3.0), sample_dtype=sdt)
    o = O.pfb(dt, h, M, cdt(3.0))
    assert bits_equal(p.execute_block(x[:300]), o.execute_block(x[:300]))
    assert bits_equal(p.execute_block(x[300:]), o.execute_block(x[300:]))
    p.push(x[5]); o.push(x[5])
    for idx in range(M):
        assert bits_equal(np.array([p.execute(idx)]), np.array([o.pfb_execute(idx)]))


@pytest.mark.parametrize("dt,cdt,sdt", DTYPES)
@pytest.mark.parametrize("L,M", [(10, 4), (64, 8), (9, 3), (5, 1)])
def test_interp_exact_bit_parity(dt, cdt, sdt, L, M):
    rng = np.random.default_rng(L * 31 + M + dt)
    h = rand(rng, L, cdt)
    x = rand(rng, 513, sdt)
    f = InterpolatingFIRFilter(h, M, sample_dtype=sdt)
    o = O.interp(dt, h, M)
    assert bits_equal(f.execute_block(x[:200]), o.execute_block(x[:200]))
    assert bits_equal(f.execute_block(x[200:]), o.execute_block(x[200:]))
    if dt in (O.RR64, O.RC64):
        for fr in (0.0, 0.05, 0.25):
            assert f.frequency_response(fr) == o.frequency_response(fr)
            assert f.group_delay(fr) == o.group_delay(fr)


def test_pfb_reset():
    rng = np.random.default_rng(3)
    h = rand(rng, 32, F64)
    x = rand(rng, 40, C128)
    p = PolyPhaseFilterBank(h, 4, 1.0, sample_dtype=C128)
    p.execute_block(x)
    p.reset()
    assert bits_equal(p.execute_block(x), O.pfb(O.RC64, h, 4, 1.0).execute_block(x))
    # clone of a plain filterbank, 3 channels, mid-stream: the window, scale and channels travel
    x3 = rand(rng, 3 * 18, C128).reshape(3, 18)
    p = PolyPhaseFilterBank(h, 4, 2.0, sample_dtype=C128, channels=3)
    p.execute_block(x3[:, :7])
    c = p.clone()
    assert c.channels == 3 and c.get_scale() == p.get_scale()
    yc = c.execute_block(x3[:, 7:])
    assert bits_equal(p.execute_block(x3[:, 7:]), yc)
    for ch in range(3):
        o = O.pfb(O.RC64, h, 4, 2.0)
        o.execute_block(x3[ch, :7])
        assert bits_equal(yc[ch], o.execute_block(x3[ch, 7:]))


# ---------------------------------------------------------------- synthetic stream
def test_device_synth_matches_host():
    import torch
    n = 1 << 20
    d = torch.empty(n, dtype=torch.float32, device="cuda")
    lib = sd.lib()
    assert lib.sdsp_synth_f32_device(d.data_ptr(), 20250226, 5, 1000, n, None) == 0
    got = to_host(d)
    ref = O.synth(20250226, 5, 1000, n)
    assert bits_equal(got, ref)


# ---------------------------------------------------------------- tiled interpolator (M = 2^m >= 8, K in {4, 8, 16})
@pytest.mark.parametrize("dt,cdt,sdt", DTYPES)
@pytest.mark.parametrize("L,M", [(32, 8), (256, 32), (60, 16), (256, 16), (4096, 512), (512, 64)])
def test_interp_tiled_exact_bit_parity(dt, cdt, sdt, L, M):
    """ragged calls across tile boundaries (T = 16 * 512 / M inputs per workgroup), K = ceil_f32(L / M)"""
    rng = np.random.default_rng(L + M + dt)
    h = rand(rng, L, cdt)
    x = rand(rng, 3001, sdt)
    f = InterpolatingFIRFilter(h, M, sample_dtype=sdt)
    assert f.subfilter_len() in (4, 8, 16)
    o = O.interp(dt, h, M)
    for a, b in [(0, 1), (1, 2), (2, 1030), (1030, 1031), (1031, 3001)]:
        assert bits_equal(f.execute_block(x[a:b]), o.execute_block(x[a:b])), (a, b)


@pytest.mark.parametrize("dt,cdt,sdt", [(O.RC32, F32, C64), (O.CC32, C64, C64), (O.RC64, F64, C128)])
def test_interp_tiled_fma_and_channels(dt, cdt, sdt):
    import torch
    rng = np.random.default_rng(dt)
    M, L, ch, n = 32, 256, 3, 5000
    h = rand(rng, L, cdt)
    x = rand(rng, ch * n, sdt).reshape(ch, n)
    f = InterpolatingFIRFilter(h, M, sample_dtype=sdt, algo=sd.ALGO_FMA, channels=ch)
    d_in = to_dev(x.reshape(-1))
    d_out = empty_dev(ch * n * M, sdt)
    f.execute_block_device(d_in[: ch * n], n, d_out)
    torch.cuda.synchronize()
    y = to_host(d_out).reshape(ch, n * M)
    tol = 1e-6 if np.dtype(sdt) == np.complex64 else 1e-13
    for c in range(ch):
        ref = O.interp(O.CC64 if np.dtype(cdt).kind == "c" else O.RC64, h.astype(C128 if np.dtype(cdt).kind == "c" else F64),
                       M).execute_block(x[c].astype(C128))
        assert rel_rms(y[c], ref) <= tol


def test_pfb_rejects_in_place():
    import torch
    f = InterpolatingFIRFilter(np.ones(64, F32), 8, sample_dtype=C64)
    buf = torch.zeros(8 * 100, dtype=torch.complex64, device="cuda")
    with pytest.raises(sd.SdspError):
        f.execute_block_device(buf, 100, buf)


# ---------------------------------------------------------------- per-sample step kernel
@pytest.mark.parametrize("dt,cdt,sdt", DTYPES)
@pytest.mark.parametrize("L,M", [(1, 1), (63, 1), (256, 1), (24, 4), (9, 3)])
def test_per_sample_execute_bit_parity(dt, cdt, sdt, L, M):
    """Filter::execute / DecimatingFIRFilter::push through the single-launch step kernel,
    interleaved with execute_block, bit-identical to the restatement"""
    rng = np.random.default_rng(L * 7 + M + dt)
    h = rand(rng, L, cdt)
    x = rand(rng, 300, sdt)
    s = cdt(0.75)
    if M == 1:
        f, o = FIRFilter(h, s, sample_dtype=sdt), O.fir(dt, h, s)
    else:
        f, o = DecimatingFIRFilter(h, s, M, sample_dtype=sdt), O.decim(dt, h, s, M)
    got, ref = [], []
    for i in range(40):  # per-sample calls
        got += list(f.execute(x[i]))
        ref += list(o.execute_block(x[i:i + 1]))
    got += list(f.execute_block(x[40:200]))
    ref += list(o.execute_block(x[40:200]))
    if M > 1:
        f.push(x[200]); o.push(x[200])
    for i in range(201, 230):
        got += list(f.execute(x[i]))
        ref += list(o.execute_block(x[i:i + 1]))
    got += list(f.execute_block(x[230:]))
    ref += list(o.execute_block(x[230:]))
    assert len(got) == len(ref)
    assert bits_equal(np.array(got, dtype=sdt), np.array(ref, dtype=sdt))


@pytest.mark.parametrize("dt,cdt,sdt", DTYPES)
@pytest.mark.parametrize("L,M,n1,n2", [(21, 3, 5000, 3333), (240, 24, 700, 9001), (3000, 1000, 9, 5),
                                       (6000, 2, 4100, 77), (12000, 2, 300, 50)])
def test_pfb_staged_kernel_bit_parity(dt, cdt, sdt, L, M, n1, n2):
    """the LDS-staged generic kernel (tiles of ~4096 outputs, coefficients staged when they fit)
    and, on the wider samples, the per-output fallback: bit-identical to the restatement over two
    calls (tile edges, history).  By pfb_route's rule (restated in tests/pfb_cases.py, these shapes
    classified in tests/test_pfb_cases.py) the first three shapes stage their branch taps in LDS
    on every pair; (6000, 2) does so on RR32 only, reads them from global memory on RC32, CC32
    and RR64 and runs the per-output kernel on RC64 and CC64; (12000, 2) runs the per-output
    kernel on every pair but RR32, which stays on the staged kernel with its taps in global
    memory (xb = 32192 bytes of samples): 4-byte samples leave it only at K >= 8194 (M = 1).
    pfb_kernel<float, float, *> and the per-output kernel on several channels are run by
    tests/test_gpu_pfb_paths.py"""
    rng = np.random.default_rng(L + M + dt)
    h = rand(rng, L, cdt)
    x = rand(rng, n1 + n2, sdt)
    p = PolyPhaseFilterBank(h, M, cdt(1.0), sample_dtype=sdt)
    o = O.pfb(dt, h, M, cdt(1.0))
    assert bits_equal(p.execute_block(x[:n1]), o.execute_block(x[:n1]))
    assert bits_equal(p.execute_block(x[n1:]), o.execute_block(x[n1:]))


def test_default_handle_is_exact_on_large_blocks():
    """A handle built without an algo runs the reference-order kernel at every block
    size: a crcf block above the 65536-sample size where AUTO would pick overlap-save
    is bit-identical to the f32 restatement (default paths never change results)."""
    rng = np.random.default_rng(65537)
    h = rng.standard_normal(256).astype(F32)
    x = rand(rng, 70000, C64)
    f = FIRFilter(h, F32(0.2), sample_dtype=C64)
    o = O.fir(O.RC32, h, F32(0.2))
    assert bits_equal(f.execute_block(x), o.execute_block(x))
    d = DecimatingFIRFilter(h, F32(0.2), 32, sample_dtype=C64)
    assert bits_equal(d.execute_block(x), O.decim(O.RC32, h, F32(0.2), 32).execute_block(x))


# ---------------------------------------------------------------- host step
@pytest.mark.parametrize("dt,cdt,sdt", DTYPES)
@pytest.mark.parametrize("L,M", [(1, 1), (5, 1), (63, 1), (256, 1), (300, 1), (24, 4), (256, 32), (9, 3)])
def test_host_step_bit_parity(dt, cdt, sdt, L, M):
    """execute(sample), push, write and small host blocks run on the host against the
    handle's delay line; device blocks (host slices above the threshold and
    device-resident blocks) run on the gfx950 kernels.  Interleaved in every order that
    moves the state between the two sides -- bit-identical to the restatement
    (fir/mod.rs:209-241, decim.rs:115-139, 221-256)."""
    import torch
    rng = np.random.default_rng(L * 13 + M + dt)
    h = rand(rng, L, cdt)
    s = cdt(0.75)
    x = rand(rng, 12000, sdt)
    if M == 1:
        f, o = _FIRFilter(h, s, sample_dtype=sdt), O.fir(dt, h, s)
    else:
        f, o = _DecimatingFIRFilter(h, s, M, sample_dtype=sdt), O.decim(dt, h, s, M)
    f.set_host_step(True, block_macs=4096)
    got, ref = [], []
    i = 0

    def per_sample(k):
        nonlocal i
        for _ in range(k):
            got.extend(f.execute(x[i]))
            ref.extend(o.execute_block(x[i:i + 1]))
            i += 1

    def host_block(k):  # below the threshold: host; above it: device kernels + host window update
        nonlocal i
        got.extend(f.execute_block(x[i:i + k]))
        ref.extend(o.execute_block(x[i:i + k]))
        i += k

    def device_block(k):  # device-resident input: the host window is re-read on the next host step
        nonlocal i
        d_in = to_dev(x[i:i + k])
        d_out = empty_dev(max(f.output_count(k), 1), sdt)
        nout = f.execute_block_device(d_in, k, d_out)
        got.extend(to_host(d_out)[:nout])
        ref.extend(o.execute_block(x[i:i + k]))
        i += k

    per_sample(17)
    host_block(3)                  # host
    host_block(4096 // L + 700)    # device (above the threshold), window fed from the host slice
    per_sample(5)
    device_block(1000)
    per_sample(M + 2)
    if M > 1:
        f.push(x[i]); o.push(x[i]); i += 1
        f.write(x[i:i + 5]); o.write(x[i:i + 5]); i += 5          # host write
        f.write(x[i:i + 3000]); o.write(x[i:i + 3000]); i += 3000  # device write
        per_sample(3)
    st, ph = f.get_state()          # host window is the newer one
    c = f.clone()                   # the clone takes the host window
    per_sample(4)
    device_block(257)
    per_sample(3)
    host_block(2)
    assert len(got) == len(ref)
    assert bits_equal(np.array(got, dtype=sdt), np.array(ref, dtype=sdt)), (L, M)
    g2 = []
    for k in range(6):  # the clone continues from the snapshot
        g2.extend(c.execute(x[100 + k]))
    # a handle restored to the snapshot gives the clone's outputs
    f.set_state(st, ph)
    g3 = []
    for k in range(6):
        g3.extend(f.execute(x[100 + k]))
    assert bits_equal(np.array(g2, dtype=sdt), np.array(g3, dtype=sdt))
    f.reset()  # a zeroed delay line and phase: a fresh restatement (its FIR objects have no reset)
    o = O.fir(dt, h, s) if M == 1 else O.decim(dt, h, s, M)
    per_sample(7)
    device_block(300)
    per_sample(2)
    assert bits_equal(np.array(got, dtype=sdt), np.array(ref, dtype=sdt))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt,cdt,sdt", [DTYPES[1], DTYPES[2], DTYPES[5]])
def test_host_step_fma_matches_device_step(dt, cdt, sdt):
    """ALGO_FMA per-sample calls: the host step fuses in the device kernels' order, so
    it is bit-identical to the one-sample device step kernel"""
    rng = np.random.default_rng(dt + 5)
    h = rand(rng, 200, cdt)
    x = rand(rng, 120, sdt)
    a = _FIRFilter(h, cdt(0.5), sample_dtype=sdt, algo=sd.ALGO_FMA, host_step=True)
    b = _FIRFilter(h, cdt(0.5), sample_dtype=sdt, algo=sd.ALGO_FMA, host_step=False)
    ya = [v for s_ in x for v in a.execute(s_)]
    yb = [v for s_ in x for v in b.execute(s_)]
    assert bits_equal(np.array(ya, dtype=sdt), np.array(yb, dtype=sdt))
    ref = O.fir(O.CC64, h.astype(C128), 0.5 + 0j).execute_block(x.astype(C128))
    assert rel_rms(ya, ref) <= 1e-6


def test_step_kernel_then_caller_stream_block():
    """a device step (host_step off) followed by execute_block_device on a
    caller stream: the block reads the delay line the step kernel wrote (L > 256, so
    the step's delay-line update spans several waves)"""
    import torch
    rng = np.random.default_rng(3)
    L = 1500
    h = rng.standard_normal(L)
    x = rand(rng, 4000, C128)
    f = FIRFilter(h, 1.0, sample_dtype=C128)  # host_step=False (module wrapper)
    o = O.fir(O.RC64, h, 1.0)
    s = torch.cuda.Stream()
    got, ref = [], []
    for r in range(3):
        seg = x[r * 1000:(r + 1) * 1000]
        for k in range(3):
            got.extend(f.execute(seg[k]))
        ref.extend(o.execute_block(seg[:3]))
        d_in = to_dev(seg[3:])
        d_out = empty_dev(997, C128)
        with torch.cuda.stream(s):
            f.execute_block_device(d_in, 997, d_out, stream=s)
        s.synchronize()
        got.extend(d_out.cpu().numpy())
        ref.extend(o.execute_block(seg[3:]))
    assert bits_equal(np.array(got, dtype=C128), np.array(ref, dtype=C128))


def test_host_step_launches_no_device_work():
    """SURVEY §8b / VERDICT r02: a per-sample call is host arithmetic against the handle's
    delay line, not a device round trip.  ADVICE r04: asserted on the library's own count of
    device work per handle (sdsp_fir_device_ops: kernel launches, async copies, history pulls
    and flushes), not on timing -- 2000 execute(sample) and 2000 decimator push calls after the
    first (which pulls the delay line to the host once) queue nothing, and a device block
    afterwards does."""
    import torch
    L_ = sd.lib()
    h = np.hanning(256)
    f = _FIRFilter(h, 1.0, sample_dtype=C128)
    x = (np.arange(2000) * 0.001).astype(C128)
    f.execute(x[0])
    ops = L_.sdsp_fir_device_ops(f._h)
    got = [f.execute(v) for v in x[1:]]
    assert L_.sdsp_fir_device_ops(f._h) == ops
    ref = O.fir(O.RC64, h, 1.0)
    ref.execute_block(x[:1])
    assert bits_equal(np.array([g[0] for g in got]), ref.execute_block(x[1:]))
    d = sd.DecimatingFIRFilter(h, 1.0, 8, sample_dtype=C128)
    d.push(x[0])
    ops = L_.sdsp_fir_device_ops(d._h)
    for v in x[1:]:
        d.push(v)
    assert L_.sdsp_fir_device_ops(d._h) == ops
    # the counter does see device work: a device-resident block, then a host step (pull)
    d_in = torch.zeros(4096, dtype=torch.complex128, device="cuda")
    d_out = torch.empty_like(d_in)
    f.execute_block_device(d_in, 4096, d_out, torch.cuda.current_stream())
    assert L_.sdsp_fir_device_ops(f._h) > ops
    g = _FIRFilter(h, 1.0, sample_dtype=C128, host_step=False)  # the device step kernel: one launch per call
    g.execute(x[0])
    o0 = L_.sdsp_fir_device_ops(g._h)
    g.execute(x[1])
    assert L_.sdsp_fir_device_ops(g._h) == o0 + 1


@pytest.mark.parametrize("algo", ["exact", "fast"])
@pytest.mark.parametrize("M", [1, 32])
def test_time_sharded_stream_on_device(algo, M):
    """SURVEY §8e time-sharding as bench.py --shard time runs it (StreamShard): segments
    of one cfg2 / cfg4 stream, each on a fresh handle after its halo (parallel.time_segment)
    with device-resident blocks, concatenate to the single-stream device output --
    bit-identical on the EXACT kernels, within the §8d tolerance on the fast ones
    (overlap-save / polyphase FMA, whose block boundaries move with the call)"""
    import torch
    from solid_dsp_amd import parallel as P
    from solid_dsp_amd.filter import firdes
    n, R = 1 << 16, 3
    x = O.synth(20250226, 0, 0, R * n, complex_=True).astype(np.complex64)
    if M == 1:
        h, s = firdes.firdes_kaiser(256, 0.1, 80.0, 0.0).astype(np.float32), np.float32(0.2)
        mk = lambda: FIRFilter(h, s, sample_dtype=np.complex64, algo=sd.ALGO_EXACT if algo == "exact" else sd.ALGO_FFT)
        halo = P.fir_halo(256)
    else:
        h, s = firdes.firdes_kaiser(256, 1.0 / 64, 80.0, 0.0).astype(np.float32), np.float32(1.0 / 32)
        mk = lambda: DecimatingFIRFilter(h, s, M, sample_dtype=np.complex64,
                                         algo=sd.ALGO_EXACT if algo == "exact" else sd.ALGO_FMA)
        halo = P.decim_halo(256, M)
    st = torch.cuda.current_stream()

    def run(f, xs):
        d_in = to_dev(xs)
        d_out = empty_dev(max(f.output_count(len(xs)), 1), np.complex64)
        k = f.execute_block_device(d_in, len(xs), d_out, st)
        return to_host(d_out)[:k]

    full = run(mk(), x)
    segs = []
    for r in range(R):
        first, hh = P.time_segment(n, r, halo)
        f = mk()
        if hh:
            run(f, x[first:r * n])  # the halo: outputs dropped
        segs.append(run(f, x[r * n:(r + 1) * n]))
    got = np.concatenate(segs)
    assert len(got) == len(full)
    if algo == "exact":
        assert bits_equal(got, full)
        # and against the f32 restatement of the whole stream (the reference order
        # at the handle's precision), not only the device's own single stream
        ref32 = (O.fir(O.RC32, h, s) if M == 1 else O.decim(O.RC32, h, s, M)).execute_block(x)
        assert bits_equal(got, ref32)
    else:
        # the fast kernels' time-sharded stream against the f64 restatement of the
        # whole stream, both §8d criteria
        x64 = x.astype(np.complex128)
        h64 = h.astype(np.float64)
        ref = (O.fir(O.RC64, h64, float(s)) if M == 1 else O.decim(O.RC64, h64, float(s), M)).execute_block(x64)
        assert len(ref) == len(got)
        assert rel_rms(got, ref) <= 1e-6, rel_rms(got, ref)
        bound = 1e-6 * np.abs(h64).sum() * float(s) * np.abs(x64).max()
        assert np.abs(got - ref).max() <= bound, (np.abs(got - ref).max(), bound)


def test_fir_fft_full_size_against_exact_kernel():
    """full-size cfg2 parity in pytest, not only bench.py's four windows.  The
    whole 2^30-sample cfg2 stream (firdes_kaiser(256, 0.1, 80), scale 0.2, device-generated) through
    the overlap-save kernel, against the EXACT kernel on the same device buffer -- which is
    bit-identical to the reference restatement at f32 (test_fir_exact_bit_parity and the KATs), so
    it stands in for the oracle at a size the CPU restatement cannot reach in a test.  The §8d
    criteria over every output: rel-RMS <= 1e-6 and max|err| <= 1e-6 * sum|h| * scale * max|x|
    (accumulated in f64, 2^26-sample chunks)."""
    import torch
    n = 1 << 30
    h = _f32_taps(256, 0.1)
    x = torch.empty(n, dtype=torch.complex64, device="cuda")
    sd.lib().sdsp_synth_f32_device(x.data_ptr(), 20250226, 0, 0, 2 * n, None)
    y_fft = torch.empty_like(x)
    f = FIRFilter(h, F32(0.2), sample_dtype=C64, algo=sd.ALGO_FFT)
    assert f.execute_block_device(x, n, y_fft) == n
    torch.cuda.synchronize()
    y_ref = torch.empty_like(x)
    g = FIRFilter(h, F32(0.2), sample_dtype=C64, algo=sd.ALGO_EXACT)
    assert g.execute_block_device(x, n, y_ref) == n
    torch.cuda.synchronize()
    num = den = 0.0
    worst = 0.0
    xmax = float(x.view(torch.float32).abs().max())
    step = 1 << 26
    for a in range(0, n, step):
        yf = y_fft[a:a + step].to(torch.complex128)
        yr = y_ref[a:a + step].to(torch.complex128)
        d = (yf - yr).abs()
        num += float((d * d).sum())
        den += float((yr.abs() ** 2).sum())
        worst = max(worst, float(d.max()))
    rel = (num / den) ** 0.5
    assert rel <= 1e-6, rel
    # |x| of a complex sample is at most sqrt(2) times its largest component
    assert worst <= 1e-6 * float(np.abs(h).sum()) * 0.2 * xmax * 2 ** 0.5, worst


@pytest.mark.parametrize("sdt,algo", [(C64, "exact"), (C64, "fft"), (C128, "exact")])
def test_fir_large_host_slice_matches_device(sdt, algo):
    """host slices of 40-48 MB (the drop-in path: H2D, one kernel call, D2H): bit-identical to
    device-resident calls over the same two consecutive slices (the delay line crossing calls),
    and the overlap-save path within the §8d tolerance of the f64 restatement"""
    import torch
    # (n even: the second device slice starts 16-byte aligned like the host path's staging buffer,
    # so both take the same overlap-save kernel form)
    n = (5 << 20) + 778 if sdt == C64 else (3 << 20) + 555
    h = _f32_taps(64, 0.1)
    cdt = F32 if sdt == C64 else F64
    rng = np.random.default_rng(31)
    x = rand(rng, 2 * n, sdt)
    a = sd.ALGO_EXACT if algo == "exact" else sd.ALGO_FFT
    f = FIRFilter(h.astype(cdt), cdt(0.2), sample_dtype=sdt, algo=a)
    y = np.concatenate([f.execute_block(x[:n]), f.execute_block(x[n:])])
    g = FIRFilter(h.astype(cdt), cdt(0.2), sample_dtype=sdt, algo=a)
    d_in = torch.from_numpy(x).to("cuda")
    d_out = torch.empty_like(d_in)
    st = torch.cuda.current_stream()
    g.execute_block_device(d_in[:n], n, d_out[:n], st)
    g.execute_block_device(d_in[n:], n, d_out[n:], st)
    torch.cuda.synchronize()
    assert bits_equal(y, d_out.cpu().numpy())
    if algo == "fft":
        ref = O.fir(O.CC64, h.astype(C128), 0.2 + 0j).execute_block(x.astype(C128))
        assert rel_rms(y, ref) <= 1e-6
        assert np.abs(y - ref).max() <= 1e-6 * np.abs(h).sum() * 0.2 * np.abs(x).max()
