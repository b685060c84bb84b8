"""Overlap-save for long filters on 32-bit complex samples (3841 < L - 1 <= 2^20, ALGO_FFT on RC32 /
CC32 handles, kern_fir_ols_long.hip): one N-point segment transform per N - (L-1) outputs in three
passes, N = N1 N2.

Reference: a complex128 FFT convolution in numpy (the stream zero-padded to a power of two >= n + L,
nothing prepended: a fresh handle's history is zero).  test_fft_reference_matches_restatement pins it
to the f64 restatement O.fir(...), so the GPU tests run no O(n L) restatement in f64.
Tolerance: the section 8d pair, as check_8d of test_gpu_fir_ols_real.py:
    rel_RMS <= 1e-6   and   max|err| <= 1e-6 * sum|h| * |scale| * max|x|.
Inputs: firdes_kaiser(L, 0.1, 80, 0) taps as f32 (CC32: times exp(2j pi 0.05 i), as complex64),
scale 0.2, streams from O.synth(..., complex_=True).
"""
import functools

import numpy as np
import pytest

import oracle_lib as O
from gpu_util import bits_equal, rel_rms, to_dev, empty_dev, to_host

gpu = pytest.mark.gpu

sd = pytest.importorskip("solid_dsp_amd")
from solid_dsp_amd import FIRFilter as _FIRFilter, DecimatingFIRFilter  # noqa: E402

F32, F64, C64, C128 = np.float32, np.float64, np.complex64, np.complex128
SCALE = 0.2
SEED = 20251101
TUNE_LOG2N, TUNE_SEGS = 22, 23
AUTO_LONG = 1 << 16  # AUTO: long-filter c32 blocks of at least this many samples take overlap-save
L0 = 3842            # the shortest filter of the long path


def FIRFilter(*a, **k):
    k.setdefault("host_step", False)
    return _FIRFilter(*a, **k)


@functools.lru_cache(maxsize=None)
def taps(L, cplx=False):
    h = O.firdes_kaiser(L, 0.1, 80.0, 0.0).astype(F32)
    if cplx:
        h = (h * np.exp(2j * np.pi * 0.05 * np.arange(L))).astype(C64)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def stream(ch, n):
    x = O.synth(SEED, ch, 0, n, complex_=True)
    x.setflags(write=False)
    return x


def fft_conv(h, scale, x):
    """y[j] = scale * sum_i h[L-1-i] x[j-i] (the stored taps are the reversed ones), x[<0] = 0,
    by a complex128 FFT convolution"""
    n, L = len(x), len(h)
    M = 1 << int(n + L - 1).bit_length()
    g = np.asarray(h)[::-1].astype(C128) * complex(scale)
    return np.fft.ifft(np.fft.fft(np.asarray(x).astype(C128), M) * np.fft.fft(g, M))[:n]


@functools.lru_cache(maxsize=None)
def reference(L, cplx, ch, n, scale=SCALE):
    ref = fft_conv(taps(L, cplx), scale, stream(ch, n))
    ref.setflags(write=False)
    return ref


def direct_window(h, scale, x, p, count):
    """outputs [p, p + count) of the same filter, summed directly in complex128 from the
    preceding inputs (zeros before the stream)"""
    L = len(h)
    lo = p - (L - 1)
    xs = np.zeros(count + L - 1, dtype=C128)
    xs[max(0, -lo):] = x[max(lo, 0):p + count]
    return np.convolve(xs, np.asarray(h)[::-1].astype(C128) * complex(scale), mode="valid")


def check_8d(y, ref, h, scale, x, what):
    rel = rel_rms(y, ref)
    err = float(np.abs(np.asarray(y).astype(C128) - ref).max())
    bound = 1e-6 * float(np.abs(np.asarray(h).astype(C128)).sum()) * abs(scale) * float(np.abs(x).max())
    print(f"{what}: rel-RMS {rel:.3e}, max|err| {err:.3e} (bound {bound:.3e})")
    assert rel <= 1e-6, f"{what}: rel-RMS {rel:.3e} > 1e-6"
    assert err <= bound, f"{what}: max|err| {err:.3e} > {bound:.3e} (rel-RMS {rel:.3e})"
    return rel


def cdt(cplx):
    return C64 if cplx else F32


def ols(L=L0, cplx=False, scale=SCALE, algo=None, **k):
    return FIRFilter(taps(L, cplx), cdt(cplx)(scale), sample_dtype=C64,
                     algo=sd.ALGO_FFT if algo is None else algo, **k)


def auto_nfft(L):
    N = 1 << 14
    while N < 4 * (L - 1):
        N *= 2
    return N


# ---------------------------------------------------------------- the reference itself
def test_fft_reference_matches_restatement():
    """the numpy FFT convolution against the f64 restatement: RC64 at n = 20000, L = 3842, and
    (for the tap order) CC64 with the asymmetric complex taps at n = 3000, L = 300"""
    h, x = taps(L0), stream(0, 20000)
    ref = O.fir(O.RC64, h.astype(F64), SCALE).execute_block(x.astype(C128))
    rel = rel_rms(fft_conv(h, SCALE, x), ref)
    print(f"RC64 L={L0}: rel-RMS {rel:.3e}")
    assert rel <= 1e-12
    hc = taps(300, True)
    refc = O.fir(O.CC64, hc.astype(C128), SCALE).execute_block(x[:3000].astype(C128))
    relc = rel_rms(fft_conv(hc, SCALE, x[:3000]), refc)
    print(f"CC64 L=300: rel-RMS {relc:.3e}")
    assert relc <= 1e-12
    relw = rel_rms(direct_window(hc, SCALE, x[:3000], 100, 500), refc[100:600])
    print(f"CC64 L=300 direct window: rel-RMS {relw:.3e}")
    assert relw <= 1e-12


# ---------------------------------------------------------------- 1. ragged streaming
@gpu
@pytest.mark.parametrize("L,cplx,ch", [(3842, False, 3), (4097, True, 1), (5000, False, 1), (5000, True, 2)])
def test_ols_long_ragged_streaming(L, cplx, ch):
    """N = 2^14 (128 x 128; L = 4097: 4 (L-1) exactly 2^14) and 2^15 (128 x 256); calls of 1 sample,
    shorter than the history, shorter than V, exactly V, 3 V + 17 and a ragged tail"""
    f = ols(L, cplx, channels=ch)
    N = auto_nfft(L)
    nfft, V = f.ols_info()
    assert (nfft, V) == (N, N - (L - 1))
    cuts = np.cumsum([0, 1, 3000, 7001, V, 3 * V + 17, 1234]).tolist()
    n = cuts[-1]
    x = np.stack([stream(c, n) for c in range(ch)]) if ch > 1 else stream(0, n)
    y = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        y.append(f.execute_block(x[..., a:b]))
        hist, _ = f.get_state()
        want = np.zeros((ch, L - 1), dtype=C64)
        k = min(b, L - 1)
        want[:, L - 1 - k:] = x.reshape(ch, -1)[:, b - k:b]
        assert bits_equal(hist, want.reshape(-1)), (a, b)
    y = np.concatenate(y, axis=-1)
    for c in range(ch):
        check_8d(y[c] if ch > 1 else y, reference(L, cplx, c, n), taps(L, cplx), SCALE, stream(c, n),
                 f"L={L} {'CC32' if cplx else 'RC32'} ch={c}/{ch}")


# ---------------------------------------------------------------- 2. rounds
@gpu
def test_ols_long_rounds():
    """two segments per round on a call of 7 V + 123 samples (four rounds, the last one ragged):
    the bits of a handle with automatic rounds"""
    a, b = ols(), ols()
    b.set_tuning(TUNE_SEGS, 2)
    _, V = a.ols_info()
    n = 7 * V + 123
    x = stream(1, n)
    ya, yb = a.execute_block(x), b.execute_block(x)
    assert bits_equal(ya, yb), "rounds of two segments differ from automatic rounds"
    check_8d(yb, reference(L0, False, 1, n), taps(L0), SCALE, x, "rounds of 2")
    for bad in (-1, 4097):
        with pytest.raises(sd.SdspError) as e:
            b.set_tuning(TUNE_SEGS, bad)
        assert e.value.code == 90


# ---------------------------------------------------------------- 3. forced transform sizes
@gpu
@pytest.mark.parametrize("lg", [13, 16, 20, 22])
def test_ols_long_forced_sizes(lg):
    """N = 2^13 (64 x 128, V / N about one half), 2^16, 2^20 (1024 x 1024), 2^22 (2048 x 2048) on
    one call of 2 V + V / 2 samples; six windows of 2048 outputs recomputed directly in complex128"""
    f = ols()
    for bad in (12, 23):
        with pytest.raises(sd.SdspError) as e:
            f.set_tuning(TUNE_LOG2N, bad)
        assert e.value.code == 90
    f.set_tuning(TUNE_LOG2N, lg)
    N, V = f.ols_info()
    assert (N, V) == (1 << lg, (1 << lg) - (L0 - 1))
    n = 2 * V + V // 2
    x = stream(2, n)
    y = f.execute_block(x)
    hist, _ = f.get_state()
    assert bits_equal(hist, x[n - (L0 - 1):])
    W = 2048
    # the last start: segment output index 1003 + 3841, not a multiple of the 16 (8, 4) columns
    # a workgroup takes
    starts = {"first": 0, "boundary 1": V - W // 2, "boundary 2": 2 * V - W // 2, "mid-segment": V + V // 2 - W // 2,
              "last": n - W, "odd column": V + 1003}
    for name, p in starts.items():
        assert 0 <= p and p + W <= n
        check_8d(y[p:p + W], direct_window(taps(L0), SCALE, x, p, W), taps(L0), SCALE, x, f"N=2^{lg} {name} [{p}, +{W})")


# ---------------------------------------------------------------- 4. device buffers
@gpu
def test_ols_long_device_buffers():
    """torch c32 tensors sliced at element offset 1 (8-byte alignment only) on torch's current
    stream; nothing written outside the output block; an overlapping pair is rejected"""
    import torch
    n = 100001
    x = stream(3, n)
    d_in = empty_dev(n + 1, C64)
    d_in[1:1 + n].copy_(to_dev(x))
    d_out = empty_dev(n + 2, C64)
    d_out.fill_(complex(float("nan"), float("nan")))
    f = ols()
    f.execute_block_device(d_in[1:1 + n], n, d_out[1:1 + n], torch.cuda.current_stream())
    out = to_host(d_out)
    assert np.isnan(out[0]) and np.isnan(out[n + 1]), "wrote outside the output block"
    check_8d(out[1:1 + n], reference(L0, False, 3, n), taps(L0), SCALE, x, "device buffers at offset 1")
    hist, _ = f.get_state()
    assert bits_equal(hist, x[n - (L0 - 1):])
    with pytest.raises(sd.SdspError) as e:
        f.execute_block_device(d_in[1:1 + n], n, d_in[0:n], torch.cuda.current_stream())
    assert e.value.code == 90


# ---------------------------------------------------------------- 5. state
@gpu
def test_ols_long_determinism_clone_reset_set_scale_state():
    cuts = [0, 20001, 33000, 46000, 60000]
    n = cuts[-1]
    x = stream(4, n)
    blk = [x[p:q] for p, q in zip(cuts[:-1], cuts[1:])]
    a, b = ols(), ols()
    ya = [a.execute_block(v) for v in blk[:2]]
    yb = [b.execute_block(v) for v in blk[:2]]
    assert all(bits_equal(u, v) for u, v in zip(ya, yb)), "two fresh handles differ"
    c = a.clone()
    assert c.ols_info() == a.ols_info()
    ya2, yc2 = a.execute_block(blk[2]), c.execute_block(blk[2])
    assert bits_equal(ya2, yc2), "clone differs"
    # get_state / set_state into a new handle, then the same next block
    hist, _ = a.get_state()
    assert bits_equal(hist, x[cuts[3] - (L0 - 1):cuts[3]])
    d = ols()
    d.set_state(hist)
    ya3, yd3 = a.execute_block(blk[3]), d.execute_block(blk[3])
    assert bits_equal(ya3, yd3), "restored handle differs"
    check_8d(np.concatenate(ya + [ya2, ya3]), reference(L0, False, 4, n), taps(L0), SCALE, x, "four calls")
    # reset, then the first block again
    a.reset()
    assert bits_equal(a.execute_block(blk[0]), ya[0]), "reset handle differs from a fresh one"
    # set_scale mid-stream: the plan is rebuilt, the history carried
    b.set_scale(F32(0.5))
    check_8d(b.execute_block(blk[2]), reference(L0, False, 4, n, 0.5)[cuts[2]:cuts[3]], taps(L0), 0.5, x,
             "after set_scale(0.5)")
    hist, _ = b.get_state()
    assert bits_equal(hist, x[cuts[3] - (L0 - 1):cuts[3]])


# ---------------------------------------------------------------- 6. mixed algorithms on one handle
@gpu
def test_ols_long_mixed_algorithms():
    """EXACT, then set_algo(FFT), then EXACT on one handle: the reference-order blocks are the f32
    restatement's bits at their positions, the overlap-save block is within section 8d"""
    cuts = [0, 5000, 25000, 30000]
    n = cuts[-1]
    x = stream(5, n)
    ref32 = O.fir(O.RC32, taps(L0), F32(SCALE)).execute_block(x)
    f = ols(algo=sd.ALGO_EXACT)
    y0 = f.execute_block(x[cuts[0]:cuts[1]])
    f.set_algo(sd.ALGO_FFT)
    y1 = f.execute_block(x[cuts[1]:cuts[2]])
    f.set_algo(sd.ALGO_EXACT)
    y2 = f.execute_block(x[cuts[2]:cuts[3]])
    assert bits_equal(y0, ref32[cuts[0]:cuts[1]]), "first EXACT block"
    assert bits_equal(y2, ref32[cuts[2]:cuts[3]]), "EXACT block after the overlap-save block"
    check_8d(y1, reference(L0, False, 5, n)[cuts[1]:cuts[2]], taps(L0), SCALE, x, "FFT block between EXACT blocks")
    assert not bits_equal(y1, ref32[cuts[1]:cuts[2]]), "the FFT block did not take the overlap-save path"


# ---------------------------------------------------------------- 7. AUTO
@gpu
def test_ols_long_auto():
    """AUTO on a long-filter RC32 handle: a block one sample short of the threshold is the f32
    restatement's bits, a block of the threshold length is ALGO_FFT's bits; RR32 stays exact"""
    n = 2 * AUTO_LONG - 1
    x = stream(6, n)
    f, g = ols(algo=sd.ALGO_AUTO), ols()
    ref32 = O.fir(O.RC32, taps(L0), F32(SCALE)).execute_block(x[:AUTO_LONG - 1])
    yf = f.execute_block(x[:AUTO_LONG - 1])
    assert bits_equal(yf, ref32), "AUTO below the threshold is not the reference-order kernel"
    g.execute_block(x[:AUTO_LONG - 1])
    yf2, yg2 = f.execute_block(x[AUTO_LONG - 1:]), g.execute_block(x[AUTO_LONG - 1:])
    assert bits_equal(yf2, yg2), "AUTO at the threshold is not the overlap-save path"
    check_8d(yf2, reference(L0, False, 6, n)[AUTO_LONG - 1:], taps(L0), SCALE, x, "AUTO at the threshold")
    xr = np.ascontiguousarray(stream(6, AUTO_LONG).real)
    r = FIRFilter(taps(L0), F32(SCALE), sample_dtype=F32, algo=sd.ALGO_AUTO)
    assert bits_equal(r.execute_block(xr), O.fir(O.RR32, taps(L0), F32(SCALE)).execute_block(xr)), "RR32 under AUTO"


# ---------------------------------------------------------------- 8. scope
@gpu
def test_ols_long_scope():
    rr = FIRFilter(taps(L0), F32(SCALE), sample_dtype=F32)
    dec = DecimatingFIRFilter(taps(L0), F32(SCALE), 2, sample_dtype=C64, host_step=False)
    big = np.zeros((1 << 20) + 2, dtype=F32)
    big[:L0] = taps(L0)
    huge = FIRFilter(big, F32(SCALE), sample_dtype=C64)
    for f in (rr, dec, huge):
        with pytest.raises(sd.SdspError) as e:
            f.set_algo(sd.ALGO_FFT)
        assert e.value.code == 91
        assert f.ols_info() == (0, 0)
        with pytest.raises(sd.SdspError) as e:  # handles outside the long scope accept only 0
            f.set_tuning(TUNE_LOG2N, 14)
        assert e.value.code == 90
        f.set_tuning(TUNE_LOG2N, 0)
    assert FIRFilter(taps(256), F32(SCALE), sample_dtype=C64).ols_info() == (4096, 3840)
    assert FIRFilter(taps(700), F32(SCALE), sample_dtype=F32).ols_info() == (4096, 4096 - 768)
    assert FIRFilter(taps(256).astype(F64), F64(SCALE), sample_dtype=C128).ols_info() == (0, 0)
    edge = FIRFilter(big[:(1 << 20) + 1], F32(SCALE), sample_dtype=C64)  # L - 1 = 2^20: in scope
    assert edge.ols_info() == (1 << 22, (1 << 22) - (1 << 20))
    edge.set_algo(sd.ALGO_FFT)
    with pytest.raises(sd.SdspError) as e:  # 2^20 < 2 (L-1)
        edge.set_tuning(TUNE_LOG2N, 20)
    assert e.value.code == 90
