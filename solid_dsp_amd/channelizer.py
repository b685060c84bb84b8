"""PFB + FFT channeliser (BASELINE config 5; build-defined composition of the
reference's PolyPhaseFilterBank coefficient layout, src/filter/fir/pfb.rs:24-49,
and FFT FORWARD, src/fft/mod.rs:175-215 — SURVEY Appendix A.6).

    v_p[m] = sum_{i<K} h[p + (K-1-i) M] x[(m-i) M + (M-1-p)]
    X[m]   = FFT_M(v[m])          (forward, unnormalised)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._handle import ChanHandle


class Channelizer(ChanHandle):
    """Knobs: L.TUNE_CHAN_STREAMING, L.TUNE_CHAN_FRAMES_PER_BLOCK, L.TUNE_CHAN_XCD_ORDER."""
    _family = "chan"

    def __init__(self, taps, channels: int, sample_dtype=np.complex64, device=0, streams=1):
        self._create(taps, channels, sample_dtype, device, streams)

    def execute_block(self, samples) -> np.ndarray:
        """[streams, n] (or [n]) samples -> [streams, n/M, M] (or [n/M, M]) channel outputs."""
        x = np.ascontiguousarray(samples, dtype=self.sample_dtype)
        n = x.shape[-1]
        out = np.zeros(x.shape[:-1] + (n // self.M, self.M), dtype=self.sample_dtype)
        fr = C.c_size_t(0)
        self._call("execute_block", L.ptr(x), n, L.ptr(out) if out.size else None, C.byref(fr))
        return out
