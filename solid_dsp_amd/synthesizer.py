"""Synthesis channeliser: M baseband channels back into one wideband stream, the counterpart of
``Channelizer`` (build-defined; the inverse FFT fused into the polyphase bank, ``kern_ichan.hip``).

    u[m]       = REVERSE_FFT_M(X[m])                              (unnormalised)
    y[m M + r] = sum_{i<K} g[r + (K-1-i) M] u[m-i][M-1-r]         K = len(g) // M

Frames before the handle's first are zero.  Fed by ``Channelizer(h, M)`` it gives
``M sum_i sum_j g[r + (K_g-1-i) M] h[(M-1-r) + (K_h-1-j) M] x[(m-i-j) M + r]`` (include/sdsp.h).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._handle import ChanHandle, info


class ChannelSynthesizer(ChanHandle):
    _family = "ichan"
    KERNELS = {1: "per_frame", 2: "ring"}

    def __init__(self, taps, channels: int, sample_dtype=np.complex64, device=0, streams=1):
        self._create(taps, channels, sample_dtype, device, streams)

    # set_tuning: L.TUNE_ICHAN_KERNEL (0 automatic, 1 per-frame, 2 ring), L.TUNE_ICHAN_FRAMES_PER_BLOCK
    info = info

    def subfilter_len(self) -> int:
        return int(L.lib().sdsp_ichan_subfilter_len(self._h))

    def execute_block(self, frames) -> np.ndarray:
        """[streams, frames, M] (or [frames, M]) channel samples -> [streams, frames*M] (or [frames*M])
        time samples."""
        x = np.ascontiguousarray(frames, dtype=self.sample_dtype)
        if x.ndim < 2 or x.shape[-1] != self.M:
            raise ValueError("input must be [frames, M] or [streams, frames, M]")
        n = x.shape[-2] * self.M
        out = np.zeros(x.shape[:-2] + (n,), dtype=self.sample_dtype)
        fr = C.c_size_t(0)
        self._call("execute_block", L.ptr(x), n, L.ptr(out) if out.size else None, C.byref(fr))
        return out
