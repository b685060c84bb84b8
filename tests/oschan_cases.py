"""Numpy restatements for the oversampled channeliser (sdsp_oschan_*, solid_dsp_amd.OversampledChannelizer)
and the inputs its tests share.  No GPU import: tests/test_oschan_capi.py pins these functions to each
other on the CPU, tests/test_gpu_oschan.py holds the handle to them.

With K = len(h) // M (later taps ignored), x[<0] = 0 and m the frame index since the handle's start:

    v_p[m] = sum_{i<K} h[p + (K-1-i) M] x[(m+1) D - 1 - p - i M]      p = 0 .. M-1
    w_q[m] = v_{(q + (m+1) D) mod M}[m]
    Y[m]   = fft(w[m])

- oschan_ref: the formulas above in complex128; it takes the index of its first frame and an initial
  history (the K M - D samples before the block), so a split call can be restated;
- oschan_exact: the rotated branch sums w bit for bit in the handle's real type, ready for an FFT;
- oschan_f32: what f32 arithmetic alone gives (numpy float32 sums behind scipy's single-precision FFT);
- ddc_form: channel k as a mix with e^{+j 2 pi k (n+1) / M}, a convolution with g and a decimation by D.
"""
from __future__ import annotations

import functools

import numpy as np

import oracle_lib as O
from ichan_cases import (AMP, C64, C128, F32, TOL, check_streams, coef_dtype, name,  # noqa: F401
                         white_taps, _rows)

SEED = 20261101  # streams
TUNE_KERNEL, TUNE_FPB = 27, 28  # SDSP_TUNE_OSCHAN_KERNEL, SDSP_TUNE_OSCHAN_FRAMES_PER_BLOCK
FRAMES = 45
BLOCKS = [1, 2, 8, 34]  # one frame; a call shorter than the history; odd frame counts at every cut


def hist_len(M, K, D):
    return K * M - D


def _gather(M, K, D, frames):
    """idx[i][f][p] = H + (f+1) D - 1 - p - i M: where frame f's branch p finds its i-th sample in
    [history, block]"""
    f = np.arange(frames)[:, None]
    p = np.arange(M)[None, :]
    return [hist_len(M, K, D) + (f + 1) * D - 1 - p - i * M for i in range(K)]


def _rotate(v, M, D, m0, shift):
    """w[f][q] = v[f][(q + sh) mod M], sh = shift(m) for the absolute frame index m = m0 + f"""
    sh = np.array([shift(m0 + f) for f in range(len(v))], dtype=np.int64)[:, None]
    return np.take_along_axis(v, (np.arange(M)[None, :] + sh) % M, axis=1)


def oschan_ref(h, M, D, x, prec=C64, m0=0, hist=None, shift=None):
    """the definition in complex128; taps and samples rounded to `prec` first.  `m0` is the index of the
    block's first frame, `hist` the K M - D samples before the block (zeros when None).  `shift`
    replaces the rotation (m+1) D (test_what_the_inputs_see).  [frames, M]"""
    hb = _rows(h, M, prec)  # hb[idx][p] = h[p + idx M]
    K, frames = len(hb), len(x) // D
    H = hist_len(M, K, D)
    past = np.zeros(H, C128) if hist is None else np.asarray(hist).astype(prec).astype(C128)
    assert len(past) == H
    xx = np.concatenate([past, np.asarray(x)[:frames * D].astype(prec).astype(C128)])
    v = np.zeros((frames, M), C128)
    for i, idx in enumerate(_gather(M, K, D, frames)):
        v += hb[K - 1 - i][None, :] * xx[idx]
    w = _rotate(v, M, D, m0, shift or (lambda m: (m + 1) * D))
    return np.fft.fft(w, axis=1)


def oschan_split(h, M, D, x, blocks, prec=C64, restart=False):
    """oschan_ref call by call: each call gets the frame index and the history the calls before it
    leave.  restart=True starts every call's frame index at 0 again (the mistake)"""
    K = len(h) // M
    H = hist_len(M, K, D)
    past, m, out, a = np.zeros(H, C128), 0, [], 0
    for nb in blocks:
        blk = np.asarray(x)[a:a + nb * D]
        out.append(oschan_ref(h, M, D, blk, prec, 0 if restart else m, past))
        past = np.concatenate([past, blk.astype(prec).astype(C128)])[len(blk):] if H else past
        m, a = m + nb, a + nb * D
    return np.concatenate(out)


def oschan_exact(h, M, D, xh, m0=0, prec=C64):
    """the handle's rotated branch sums w, bit for bit, on `xh` = the K M - D history samples followed
    by the block (dtype `prec`): real and imaginary parts as separate arrays of the handle's real type,
    a zero accumulator, i = 0 .. K-1, acc = acc + c * v (numpy rounds the product and the sum
    separately).  [frames, M] of dtype `prec`, ready for an FFT"""
    T = coef_dtype(prec)
    K = len(h) // M
    hb = np.asarray(h)[:K * M].astype(T).reshape(K, M)
    xh = np.asarray(xh)
    H = hist_len(M, K, D)
    assert xh.dtype == prec and xh.ndim == 1 and (len(xh) - H) % D == 0
    frames = (len(xh) - H) // D
    re, im = np.ascontiguousarray(xh.real), np.ascontiguousarray(xh.imag)
    ar, ai = np.zeros((frames, M), T), np.zeros((frames, M), T)
    for i, idx in enumerate(_gather(M, K, D, frames)):
        c = hb[K - 1 - i][None, :]
        ar = ar + c * re[idx]
        ai = ai + c * im[idx]
    assert ar.dtype == T and ai.dtype == T
    v = np.empty((frames, M), prec)
    v.real, v.imag = ar, ai
    return _rotate(v, M, D, m0, lambda m: (m + 1) * D)


def oschan_f32(h, M, D, x):
    """oschan_ref's sums in numpy float32 behind scipy's single-precision FFT"""
    import scipy.fft
    K = len(h) // M
    hb = np.asarray(h)[:K * M].astype(F32).reshape(K, M)
    frames = len(x) // D
    xx = np.concatenate([np.zeros(hist_len(M, K, D), C64), np.asarray(x)[:frames * D].astype(C64)])
    v = np.zeros((frames, M), C64)
    for i, idx in enumerate(_gather(M, K, D, frames)):
        v = v + hb[K - 1 - i][None, :] * xx[idx]
    assert v.dtype == C64
    y = scipy.fft.fft(_rotate(v, M, D, 0, lambda m: (m + 1) * D), axis=1)
    assert y.dtype == C64
    return y


def ddc_taps(h, M, prec=C64):
    """g[p + i M] = h[p + (K-1-i) M], f64"""
    return _rows(h, M, prec)[::-1].reshape(-1)


def ddc_form(h, M, D, x, prec=C64, channels=None):
    """every channel as a down-converter, complex128: z_k[n] = x[n] e^{+j 2 pi k (n+1) / M},
    Y[m][k] = (g * z_k)[(m+1) D - 1] with x[<0] = 0.  Only the kept outputs of the convolution are
    formed (test_ddc_form_is_a_convolution holds that to np.convolve).  [frames, len(channels)]"""
    g = ddc_taps(h, M, prec)
    L, frames = len(g), len(x) // D
    xx = np.asarray(x)[:frames * D].astype(prec).astype(C128)
    n = np.arange(len(xx))
    # win[m][t] = index of z[(m+1) D - 1 - t] in [L zeros, z]
    win = L + (np.arange(frames)[:, None] + 1) * D - 1 - np.arange(L)[None, :]
    ks = range(M) if channels is None else channels
    out = np.empty((frames, len(ks)), C128)
    for c, k in enumerate(ks):
        z = np.concatenate([np.zeros(L, C128), xx * np.exp(2j * np.pi * ((k * (n + 1)) % M) / M)])
        out[:, c] = z[win] @ g
    return out


# ---------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def white_streams(S, n, prec=C64, first=0):
    """[S, n] white samples from O.synth"""
    x = np.stack([O.synth(SEED, first + s, 0, n, complex_=True) for s in range(S)]).astype(prec)
    x.setflags(write=False)
    return x


def taps_len(M, K):
    return M * K + (M // 2 + 1 if K == 3 else 0)  # K = 3: a tail that must be ignored


@functools.lru_cache(maxsize=None)
def white_case(M, K, D, S, frames=FRAMES, prec=C64):
    """(taps, [S, frames D] streams, [S, frames, M] oschan_ref), shared by the cases of one shape"""
    h = white_taps(taps_len(M, K), prec)
    x = white_streams(S, frames * D, prec)
    ref = np.stack([oschan_ref(h, M, D, x[s], prec) for s in range(S)])
    ref.setflags(write=False)
    return h, x, ref


def slide_fits(M, K, D, prec):
    """oschan_plan's rule: the ring (K M + D samples) and the Stockham pair (2 M) within 128 KiB"""
    return (K * M + D + 2 * M) * np.dtype(prec).itemsize <= 128 * 1024


def auto_slides(M, K, D, prec):
    """oschan_plan's automatic choice: the sliding kernel where ring, pair and twiddle table take at
    most 16 KiB (measured faster than the per-frame kernel up to there)"""
    return (K * M + D + 3 * M) * np.dtype(prec).itemsize <= 16 * 1024


def auto_frames(M, K, D):
    """oschan_plan's automatic frames per workgroup: max(32, 2 ceil((K M - D) / D))"""
    return max(32, 2 * -(-hist_len(M, K, D) // D))
