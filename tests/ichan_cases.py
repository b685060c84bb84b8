"""Numpy restatements for the synthesis channeliser (sdsp_ichan_*, solid_dsp_amd.ChannelSynthesizer)
and the inputs its tests share.  No GPU import: tests/test_ichan_capi.py pins these functions to each
other on the CPU, tests/test_gpu_ichan.py holds the handle to them.

With K = len(g) // M (later taps ignored) and frames before the first equal to zero:

    u[m]       = M * ifft(X[m])                               (e^{+j 2 pi k q / M}, unnormalised)
    y[m M + r] = sum_{i<K} g[r + (K-1-i) M] * u[m-i][M-1-r]   r = 0 .. M-1

- chan_ref: the analysis channeliser, as in tests/test_gpu_chan_shapes.py;
- ichan_ref: the formulas above in complex128;
- ichan_exact: the bit-exact restatement, on frames that are already transformed;
- ichan_f32: what f32 arithmetic alone gives (numpy float32 sums behind scipy's single-precision FFT);
- pair_identity: Channelizer(h, M) feeding ChannelSynthesizer(g, M), in closed form.
"""
from __future__ import annotations

import functools

import numpy as np

import oracle_lib as O
from gpu_util import rel_rms

F32, F64, C64, C128 = np.float32, np.float64, np.complex64, np.complex128
SEED = 20261022      # frames and streams
TAP_SEED = 20261023  # white taps
AMP = 0.75 - 0.5j    # the impulse: exact in f32
TOL = {C64: 1e-6, C128: 1e-12}  # section 8d
TUNE_KERNEL, TUNE_FPB = 25, 26  # SDSP_TUNE_ICHAN_KERNEL, SDSP_TUNE_ICHAN_FRAMES_PER_BLOCK


def coef_dtype(prec):
    return F32 if prec == C64 else F64


def name(prec):
    return "c64" if prec == C64 else "c128"


def _rows(t, M, prec):
    """[K, M] f64 with rows[idx][r] = t[r + idx M], taps rounded to the precision's real type"""
    K = len(t) // M
    return np.asarray(t)[:K * M].astype(coef_dtype(prec)).astype(F64).reshape(K, M)


# ---------------------------------------------------------------- restatements
def chan_ref(h, M, x, prec=C64):
    """v_p[m] = sum_{i<K} h[p + (K-1-i) M] x[(m-i) M + (M-1-p)],  X[m] = fft(v[m]),  x[<0] = 0;
    taps and samples rounded to `prec`, then complex128.  [frames, M]"""
    hb = _rows(h, M, prec)
    K, frames = len(hb), len(x) // M
    xx = np.concatenate([np.zeros((K - 1) * M, C128), np.asarray(x)[:frames * M].astype(prec).astype(C128)])
    xr = xx.reshape(frames + K - 1, M)[:, ::-1]  # xr[f + K-1][p] = x[f M + M-1-p]
    v = np.zeros((frames, M), C128)
    for i in range(K):
        v += hb[K - 1 - i][None, :] * xr[K - 1 - i:K - 1 - i + frames]
    return np.fft.fft(v, axis=1)


def ichan_ref(g, M, X, prec=C64, flip=True):
    """the definition in complex128 on [frames, M] channel samples; taps and samples rounded to `prec`
    first.  [frames * M].  flip=False leaves out the M-1-r reversal (test_what_the_inputs_see)"""
    gb = _rows(g, M, prec)
    K = len(gb)
    X = np.asarray(X).astype(prec).astype(C128).reshape(-1, M)
    frames = len(X)
    u = np.fft.ifft(X, axis=1) * M
    uu = np.concatenate([np.zeros((K - 1, M), C128), u])  # uu[f + K-1] = u[f]
    ur = uu[:, ::-1] if flip else uu
    y = np.zeros((frames, M), C128)
    for i in range(K):
        y += gb[K - 1 - i][None, :] * ur[K - 1 - i:K - 1 - i + frames]
    return y.reshape(-1)


def ichan_exact(g, M, U, prec=C64):
    """the handle's branch sums, bit for bit, on TRANSFORMED frames U [K-1 + frames, M] of dtype `prec`
    (the first K-1 precede the first output frame): real and imaginary parts as separate arrays of the
    handle's real type, a zero accumulator, i = 0 .. K-1, acc = acc + c * v (numpy rounds the product
    and the sum separately).  [frames * M]"""
    T = coef_dtype(prec)
    K = len(g) // M
    gb = np.asarray(g)[:K * M].astype(T).reshape(K, M)
    U = np.asarray(U)
    assert U.dtype == prec and U.ndim == 2 and U.shape[1] == M and len(U) >= K
    frames = len(U) - (K - 1)
    ur = U[:, ::-1]
    re, im = np.ascontiguousarray(ur.real), np.ascontiguousarray(ur.imag)
    ar, ai = np.zeros((frames, M), T), np.zeros((frames, M), T)
    for i in range(K):
        c = gb[K - 1 - i][None, :]
        ar = ar + c * re[K - 1 - i:K - 1 - i + frames]
        ai = ai + c * im[K - 1 - i:K - 1 - i + frames]
    assert ar.dtype == T and ai.dtype == T
    out = np.empty((frames, M), prec)
    out.real, out.imag = ar, ai
    return out.reshape(-1)


def ichan_f32(g, M, X):
    """ichan_ref's sums in numpy float32 behind scipy's single-precision inverse FFT (unnormalised)"""
    import scipy.fft
    K = len(g) // M
    gb = np.asarray(g)[:K * M].astype(F32).reshape(K, M)
    X = np.asarray(X).astype(C64).reshape(-1, M)
    frames = len(X)
    u = scipy.fft.ifft(X, axis=1, norm="forward")
    assert u.dtype == C64
    ur = np.concatenate([np.zeros((K - 1, M), C64), u])[:, ::-1]
    y = np.zeros((frames, M), C64)
    for i in range(K):
        y = y + gb[K - 1 - i][None, :] * ur[K - 1 - i:K - 1 - i + frames]
    assert y.dtype == C64
    return y.reshape(-1)


def pair_identity(g, h, M, x, prec=C64):
    """Channelizer(h, M) feeding ChannelSynthesizer(g, M), in closed form and complex128:
    y[m M + r] = M sum_{i<K_g} sum_{j<K_h} g[r + (K_g-1-i) M] h[(M-1-r) + (K_h-1-j) M] x[(m-i-j) M + r]"""
    gb, hb = _rows(g, M, prec), _rows(h, M, prec)
    Kg, Kh, frames = len(gb), len(hb), len(x) // M
    lead = Kg + Kh - 2
    xx = np.concatenate([np.zeros(lead * M, C128), np.asarray(x)[:frames * M].astype(prec).astype(C128)])
    xx = xx.reshape(frames + lead, M)  # xx[f + lead][r] = x[f M + r]
    y = np.zeros((frames, M), C128)
    for i in range(Kg):
        for j in range(Kh):
            y += gb[Kg - 1 - i][None, :] * hb[Kh - 1 - j][None, ::-1] * xx[lead - i - j:lead - i - j + frames]
    return M * y.reshape(-1)


# ---------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def white_taps(n, prec=C64, seed=TAP_SEED):
    h = np.random.default_rng(seed).standard_normal(n).astype(coef_dtype(prec))
    h.setflags(write=False)
    return h


def taps_len(M, K):
    return M * K + (M // 2 + 1 if K == 5 else 0)  # K = 5: a tail that must be ignored


@functools.lru_cache(maxsize=None)
def white_frames(S, frames, M, prec=C64, first=0):
    """[S, frames, M] white channel samples from O.synth"""
    X = np.stack([O.synth(SEED, first + s, 0, frames * M, complex_=True) for s in range(S)]).astype(prec)
    X = X.reshape(S, frames, M)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def white_case(M, ntaps, S, frames, prec=C64):
    """(taps, [S, frames, M] channel samples, [S, frames * M] ichan_ref), shared by the cases of one shape"""
    g = white_taps(ntaps, prec)
    X = white_frames(S, frames, M, prec)
    ref = np.stack([ichan_ref(g, M, X[s], prec) for s in range(S)])
    ref.setflags(write=False)
    return g, X, ref


def blocks_a(K):
    return [1, K + 2, 2, 4]  # a one-frame call; calls shorter than the K-1 history frames; four calls


# ---------------------------------------------------------------- the two criteria
def figures(y, ref, M):
    """(whole-stream rel-RMS, worst frame error over the RMS frame norm, that frame) of one stream [n]"""
    y, ref = np.asarray(y).astype(C128).reshape(-1, M), np.asarray(ref).reshape(-1, M)
    err = np.linalg.norm(y - ref, axis=-1)
    rms_frame = float(np.sqrt(np.mean(np.linalg.norm(ref, axis=-1) ** 2)))
    return rel_rms(y, ref), float(err.max()) / rms_frame, int(err.argmax())


def check_streams(y, ref, M, tol, what):
    """both criteria on every stream of [S, n]; prints the worst figures of the case"""
    assert y.shape == ref.shape, (y.shape, ref.shape)
    figs = [figures(y[s], ref[s], M) for s in range(len(ref))]
    whole, frame = max(f[0] for f in figs), max(f[1] for f in figs)
    print(f"{what}: whole {whole:.3e}, frame {frame:.3e} (limit {tol:.0e})")
    for s, (w, f, m) in enumerate(figs):
        assert w <= tol, f"{what}: stream {s} rel-RMS {w:.3e} > {tol:.0e}"
        assert f <= tol, f"{what}: stream {s} frame {m} is off by {f:.3e} of the RMS frame norm > {tol:.0e}"
    return whole, frame
