"""GPU tests for overlap-save on real f32 streams with real f32 taps (FIRFilter<f32, f32> under
ALGO_FFT, kern_fir_ols_real.hip): pairs of adjacent 4096-sample real segments run as one complex
segment of the c32 transform.

Reference: the f64 restatement O.fir(O.RR64, ...) on the same f32-representable operands.
Tolerance: the §8d pair, as in test_fir_fft_tolerance:
    rel_RMS <= 1e-6   and   max|err| <= 1e-6 * sum|h| * |scale| * max|x|.
"""
import functools

import numpy as np
import pytest

import oracle_lib as O
from gpu_util import bits_equal, rel_rms, to_dev, empty_dev, to_host

pytestmark = pytest.mark.gpu

sd = pytest.importorskip("solid_dsp_amd")
from solid_dsp_amd import FIRFilter as _FIRFilter, DecimatingFIRFilter  # noqa: E402

F32, F64 = np.float32, np.float64
SCALE = 0.2
LANES4, LANES8 = 0, 3  # SDSP_TUNE_OLS_KERNEL on an RR32 handle: 4-byte lanes (default), 8-byte lanes
TUNE_OLS_KERNEL = 14
SEED = 20250301


def FIRFilter(*a, **k):
    k.setdefault("host_step", False)
    return _FIRFilter(*a, **k)


@functools.lru_cache(maxsize=None)
def taps(L):
    h = O.firdes_kaiser(L, 0.1, 80.0, 0.0).astype(F32)
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def stream(ch, n):
    x = O.synth(SEED, ch, 0, n)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(L, ch, n, scale=SCALE):
    ref = O.fir(O.RR64, taps(L).astype(F64), scale).execute_block(stream(ch, n).astype(F64))
    ref.setflags(write=False)
    return ref


def ols(L, scale=SCALE, kern=LANES4, **k):
    f = FIRFilter(taps(L), F32(scale), sample_dtype=F32, algo=sd.ALGO_FFT, **k)
    f.set_tuning(TUNE_OLS_KERNEL, kern)
    return f


def check_8d(y, ref, h, scale, x, what):
    rel = rel_rms(y, ref)
    err = float(np.abs(y.astype(F64) - ref).max())
    bound = 1e-6 * float(np.abs(h.astype(F64)).sum()) * abs(scale) * float(np.abs(x).max())
    print(f"{what}: rel-RMS {rel:.3e}, max|err| {err:.3e} (bound {bound:.3e})")
    assert rel <= 1e-6, f"{what}: rel-RMS {rel:.3e} > 1e-6"
    assert err <= bound, f"{what}: max|err| {err:.3e} > {bound:.3e} (rel-RMS {rel:.3e})"
    return rel


def halo_rows(L):
    return -(-(L - 1) // 256)


# ---------------------------------------------------------------- 1. ragged streaming
@pytest.mark.parametrize("kern", [LANES4, LANES8])
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("L", [2, 256, 257, 700, 3841])
def test_ols_real_ragged_streaming(L, ch, kern):
    """h2 = 1, 1, 2, 3, 15; calls of n = 1, shorter than the history, shorter than one window,
    with odd and even segment counts, and with the interior launch; with ch = 3 the odd call
    lengths put channel bases at odd float offsets (the 8-byte lanes then run as 4-byte ones)"""
    n = 300000
    x = np.stack([stream(c, n) for c in range(ch)]) if ch > 1 else stream(0, n)
    f = ols(L, kern=kern, channels=ch)
    cuts = [0, 1, 3000, 7001, 70002, 207714, 207715, 300000]
    y = np.concatenate([f.execute_block(x[..., a:b]) for a, b in zip(cuts[:-1], cuts[1:])], axis=-1)
    hist, _ = f.get_state()
    assert bits_equal(hist, np.ascontiguousarray(x[..., n - (L - 1):]).reshape(-1))
    for c in range(ch):
        check_8d(y[c] if ch > 1 else y, reference(L, c, n), taps(L), SCALE, stream(c, n), f"L={L} ch={c}/{ch} kern={kern}")


# ---------------------------------------------------------------- 2. whole pairs and segments
@pytest.mark.parametrize("kern", [LANES4, LANES8])
@pytest.mark.parametrize("L", [256, 700])
def test_ols_real_whole_pairs_and_segments(L, kern):
    """blocks of exactly V (one segment, B absent), 2V (one full pair ending at the block end),
    3V (odd count) and 40V samples, then a ragged tail; the history after every block"""
    V = 4096 - 256 * halo_rows(L)
    cuts = np.cumsum([0, V, 2 * V, 3 * V, 40 * V, 1235]).tolist()
    n = cuts[-1]
    x = stream(1, n)
    f = ols(L, kern=kern)
    y = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        y.append(f.execute_block(x[a:b]))
        hist, _ = f.get_state()
        assert bits_equal(hist, x[b - (L - 1):b]), (a, b)
    check_8d(np.concatenate(y), reference(L, 1, n), taps(L), SCALE, x, f"L={L} kern={kern}")


# ---------------------------------------------------------------- 3. unaligned device buffers
@pytest.mark.parametrize("kern", [LANES4, LANES8])
@pytest.mark.parametrize("off_in,off_out", [(1, 0), (0, 1)])
def test_ols_real_unaligned_device_buffers(off_in, off_out, kern):
    """device tensors sliced at element offset 1 (4-byte alignment only), input and output apart"""
    import torch
    L, n = 256, 100001
    x = stream(2, n)
    d_in = empty_dev(n + 1, F32)
    d_in[off_in:off_in + n].copy_(to_dev(x))
    d_out = empty_dev(n + 1, F32)
    d_out.fill_(float("nan"))
    f = ols(L, kern=kern)
    f.execute_block_device(d_in[off_in:off_in + n], n, d_out[off_out:off_out + n], torch.cuda.current_stream())
    out = to_host(d_out)
    y, spare = out[off_out:off_out + n], out[n if off_out == 0 else 0]
    assert np.isnan(spare), "wrote outside the output block"
    check_8d(y, reference(L, 2, n), taps(L), SCALE, x, f"offsets in={off_in} out={off_out} kern={kern}")
    hist, _ = f.get_state()
    assert bits_equal(hist, x[n - (L - 1):])


# ---------------------------------------------------------------- 4. independence of the halves
def test_ols_real_loud_and_quiet_halves():
    """second half of the stream scaled by 1e-3, the step mid-segment: the global §8d bounds hold.
    The quiet half's own rel-RMS is printed, not asserted: the rounding error of a segment is
    relative to the energy of its pair, so the quiet samples that share a transform with loud
    ones read 8.9e-5 against their own energy, the quiet pairs after them 2.2e-7 (measured)."""
    L, n = 256, 200000
    V = 4096 - 256
    step = 26 * V + 1900  # inside segment 26 (the A half of pair 13)
    x = stream(3, n).copy()
    x[step:] *= F32(1e-3)
    h = taps(L)
    ref = O.fir(O.RR64, h.astype(F64), SCALE).execute_block(x.astype(F64))
    y = ols(L).execute_block(x)
    check_8d(y, ref, h, SCALE, x, "loud + quiet")
    q0 = step + L  # past the loud samples' reach
    for name, a, b in [("quiet half", q0, n), ("quiet rest of the step's pair", q0, 28 * V),
                       ("quiet half after the step's pair", 28 * V, n)]:
        print(f"{name}: rel-RMS {rel_rms(y[a:b], ref[a:b]):.3e}")


# ---------------------------------------------------------------- 5. determinism and state
def test_ols_real_determinism_clone_reset_set_scale():
    L, n = 256, 150000
    x = stream(4, n)
    cuts = [0, 50001, 90000, n]
    a, b = ols(L), ols(L)
    ya = [a.execute_block(x[p:q]) for p, q in zip(cuts[:2], cuts[1:3])]
    yb = [b.execute_block(x[p:q]) for p, q in zip(cuts[:2], cuts[1:3])]
    assert all(bits_equal(u, v) for u, v in zip(ya, yb)), "two fresh handles differ"
    # clone mid-stream, then the same next block on both
    c = a.clone()
    ya3, yc3 = a.execute_block(x[cuts[2]:]), c.execute_block(x[cuts[2]:])
    assert bits_equal(ya3, yc3), "clone differs"
    check_8d(np.concatenate(ya + [ya3]), reference(L, 4, n), taps(L), SCALE, x, "three calls")
    # reset, then the first block again
    a.reset()
    assert bits_equal(a.execute_block(x[:cuts[1]]), ya[0]), "reset handle differs from a fresh one"
    # set_scale mid-stream: the plan is rebuilt, the history carried
    b.set_scale(F32(0.5))
    yb3 = b.execute_block(x[cuts[2]:])
    ref5 = reference(L, 4, n, 0.5)[cuts[2]:]
    check_8d(yb3, ref5, taps(L), 0.5, x, "after set_scale(0.5)")


# ---------------------------------------------------------------- 6. scope
@pytest.mark.parametrize("cdt,sdt", [(F64, F64), (F64, np.complex128), (np.complex128, np.complex128)])
def test_ols_real_scope_f64_still_unsupported(cdt, sdt):
    f = FIRFilter(taps(256).astype(cdt), cdt(SCALE), sample_dtype=sdt)
    with pytest.raises(sd.SdspError) as e:
        f.set_algo(sd.ALGO_FFT)
    assert e.value.code == 91


def test_ols_real_scope_decimator_unsupported():
    d = DecimatingFIRFilter(taps(256), F32(SCALE), 2, sample_dtype=F32, host_step=False)
    with pytest.raises(sd.SdspError) as e:
        d.set_algo(sd.ALGO_FFT)
    assert e.value.code == 91


def test_ols_real_auto_unchanged():
    """ALGO_AUTO on an RR32 handle stays the reference-order kernel: bit-equal to the f32
    restatement on a 2^17 block (at which AUTO moves c32 handles to overlap-save)"""
    n = 1 << 17
    x = stream(5, n)
    f = FIRFilter(taps(256), F32(SCALE), sample_dtype=F32, algo=sd.ALGO_AUTO)
    ref32 = O.fir(O.RR32, taps(256), F32(SCALE)).execute_block(x)
    assert bits_equal(f.execute_block(x), ref32)
    g = ols(256)  # and the overlap-save path is a different computation: within §8d, not these bits
    check_8d(g.execute_block(x), reference(256, 5, n), taps(256), SCALE, x, "ALGO_FFT 2^17")
