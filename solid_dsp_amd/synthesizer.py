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
from ._handle import Handle


class ChannelSynthesizer(Handle):
    _family = "ichan"
    KERNELS = {1: "per_frame", 2: "ring"}

    def __init__(self, taps, channels: int, sample_dtype=np.complex64, device=0, streams=1):
        sdt = np.dtype(sample_dtype)
        self.dtype = L.RC32 if sdt == np.complex64 else L.RC64
        self.coef_dtype = L.COEF_DTYPE[self.dtype]
        self.sample_dtype = L.SAMPLE_DTYPE[self.dtype]
        t = np.ascontiguousarray(taps, dtype=self.coef_dtype)
        h = C.c_void_p()
        L.check(L.lib().sdsp_ichan_create(C.byref(h), self.dtype, L.ptr(t) if len(t) else None, len(t), channels,
                                          device))
        self._h = h
        self.M = channels
        self.device = device
        self.streams = 1
        if streams != 1:
            self.set_streams(streams)

    def set_tuning(self, key: int, value: int):
        """Kernel-variant knobs (L.TUNE_ICHAN_KERNEL: 0 automatic, 1 per-frame, 2 ring;
        L.TUNE_ICHAN_FRAMES_PER_BLOCK; performance only, same bits)."""
        self._call("set_tuning", int(key), int(value))

    def set_streams(self, streams: int):
        """zeroes the history"""
        self._call("set_streams", streams)
        self.streams = streams

    def reset(self):
        self._call("reset")

    def subfilter_len(self) -> int:
        return int(L.lib().sdsp_ichan_subfilter_len(self._h))

    def info(self):
        """(kernel, frames_per_block): the kernel the next call runs (1 per-frame, 2 ring) and the ring
        kernel's frames per workgroup on a long block"""
        k, f = C.c_int(), C.c_size_t()
        self._call("info", C.byref(k), C.byref(f))
        return k.value, f.value

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

    def execute_block_device(self, d_in, n: int, d_out, stream=None) -> int:
        """Device-resident block of n = frames * M samples per stream; returns the frame count."""
        fr = C.c_size_t(0)
        pin = L.device_ptr(d_in, self.sample_dtype, self.streams * n, self.device, "input")
        pout = L.device_ptr(d_out, self.sample_dtype, self.streams * n, self.device, "output")
        self._call("execute_block_device", pin, n, pout, C.byref(fr), L.stream_handle(stream))
        return fr.value

    def synchronize(self):
        self._call("synchronize")
