"""Oversampled analysis channeliser: M channels, one frame every D <= M samples (build-defined;
``Channelizer`` is the critically sampled case D = M; ``kern_oschan.hip``).

    v_p[m] = sum_{i<K} h[p + (K-1-i) M] x[(m+1) D - 1 - p - i M]      K = len(h) // M
    w_q[m] = v_{(q + (m+1) D) mod M}[m]                               (an index rotation)
    Y[m]   = FORWARD_FFT_M(w[m])                                      (unnormalised)

Samples before the handle's first are zero and m counts frames since create / reset / set_streams.
Channel k is a down-converter: x mixed with e^{+j 2 pi k (n+1) / M}, filtered by
g[p + i M] = h[p + (K-1-i) M] and decimated by D, with a phase-continuous oscillator (include/sdsp.h).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._handle import ChanHandle, info


class OversampledChannelizer(ChanHandle):
    _family = "oschan"
    KERNELS = {1: "per_frame", 2: "sliding"}

    def __init__(self, taps, channels: int, decimation: int, sample_dtype=np.complex64, device=0, streams=1):
        self._create(taps, channels, sample_dtype, device, streams, decimation)
        self.D = decimation

    # set_tuning: L.TUNE_OSCHAN_KERNEL (0 automatic, 1 per-frame, 2 sliding), L.TUNE_OSCHAN_FRAMES_PER_BLOCK
    info = info

    @property
    def K(self) -> int:
        return int(L.lib().sdsp_oschan_subfilter_len(self._h))

    @property
    def phase(self) -> int:
        """(frames so far * D) mod M"""
        return int(L.lib().sdsp_oschan_phase(self._h))

    def execute_block(self, samples) -> np.ndarray:
        """[streams, n] (or [n]) time samples, n a multiple of D -> [streams, n/D, M] (or [n/D, M])"""
        x = np.ascontiguousarray(samples, dtype=self.sample_dtype)
        if not (x.ndim == 1 and self.streams == 1 or x.ndim == 2 and x.shape[0] == self.streams):
            raise ValueError("input must be [streams, n] (or [n] on a single-stream handle)")
        n = x.shape[-1]
        out = np.zeros(x.shape[:-1] + (n // self.D, self.M), dtype=self.sample_dtype)
        fr = C.c_size_t(0)
        self._call("execute_block", L.ptr(x) if x.size else None, n, L.ptr(out) if out.size else None, C.byref(fr))
        return out
