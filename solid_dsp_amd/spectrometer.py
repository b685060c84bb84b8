"""Spectrometer: integrated power spectra of a stream, |Y|^2 of ``OversampledChannelizer``'s frames summed
inside the kernel (build-defined; ``kern_spec.hip``).

    Y[m]    = frame m of OversampledChannelizer(taps, M, D): the same bits
    p[m][k] = Y.re Y.re + Y.im Y.im
    P_j[k]  = scale * sum of p[m][k] over frames m = jA .. jA + A - 1

summed in sub-blocks of 32 frames counted from frame jA, then over the sub-blocks, both in order
(include/sdsp.h has the exact order).  The handle keeps the open integration across calls, so a stream
of any length integrates in O(M) memory.

K = 1 with taps = a window of M points is Welch's method at hop D (overlap M - D); K > 1 is the
polyphase spectrometer.  Tap p weights the sample p back from the newest of a frame, which is
immaterial for symmetric windows.  1 <= A <= 32768: longer integrations are the caller's sum of
finished spectra.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from ._handle import ChanHandle


class Spectrometer(ChanHandle):
    _family = "spec"
    KERNELS = {1: "per_frame", 2: "sliding"}

    def __init__(self, taps, channels: int, decimation: int, integration: int, sample_dtype=np.complex64, device=0,
                 streams=1):
        self._create(taps, channels, sample_dtype, device, streams, decimation, integration)
        self.D = decimation
        self.A = integration
        self.real_dtype = self.coef_dtype

    # set_tuning: L.TUNE_SPEC_KERNEL (0 automatic, 1 per-frame, 2 sliding), L.TUNE_SPEC_SUBBLOCKS
    def info(self):
        """(kernel, subblocks_per_workgroup): the kernel the next call runs (KERNELS) and its sub-blocks of
        up to 32 frames per workgroup on a long block"""
        k, f = C.c_int(), C.c_size_t()
        self._call("info", C.byref(k), C.byref(f))
        return k.value, f.value

    @property
    def K(self) -> int:
        return int(L.lib().sdsp_spec_subfilter_len(self._h))

    @property
    def phase(self) -> int:
        """(frames so far * D) mod M"""
        return int(L.lib().sdsp_spec_phase(self._h))

    @property
    def filled(self) -> int:
        """frames in the open integration"""
        return int(L.lib().sdsp_spec_filled(self._h))

    def set_scale(self, scale: float):
        """rounded to the real dtype; applies to spectra completed afterwards and survives reset"""
        self._call("set_scale", float(scale))

    @staticmethod
    def count(decimation: int, integration: int, filled: int, n: int):
        """(spectra, next_filled) of a block of n samples per stream that starts `filled` frames into an
        integration; no handle, no device"""
        sp, nf = C.c_size_t(0), C.c_size_t(0)
        L.check(L.lib().sdsp_spec_count(decimation, integration, filled, n, C.byref(sp), C.byref(nf)))
        return sp.value, nf.value

    def execute_block(self, samples) -> np.ndarray:
        """[streams, n] (or [n]) time samples, n a multiple of D -> [streams, spectra, M] (or [spectra, M])
        in the real dtype"""
        x = np.ascontiguousarray(samples, dtype=self.sample_dtype)
        if not (x.ndim == 1 and self.streams == 1 or x.ndim == 2 and x.shape[0] == self.streams):
            raise ValueError("input must be [streams, n] (or [n] on a single-stream handle)")
        n = x.shape[-1]
        spectra = (self.filled + n // self.D) // self.A
        out = np.zeros(x.shape[:-1] + (spectra, self.M), dtype=self.real_dtype)
        sp = C.c_size_t(0)
        self._call("execute_block", L.ptr(x) if x.size else None, n, L.ptr(out) if out.size else None, C.byref(sp))
        return out

    def execute_block_device(self, d_in, n: int, d_out, stream=None) -> int:
        """Device-resident block: [streams, n] samples in, [streams, spectra, M] reals out (d_out may be
        None when the call emits nothing).  Returns the spectra count."""
        spectra = (self.filled + n // self.D) // self.A
        sp = C.c_size_t(0)
        pin = L.device_ptr(d_in, self.sample_dtype, self.streams * n, self.device, "input")
        pout = None if d_out is None else L.device_ptr(d_out, self.real_dtype, self.streams * spectra * self.M,
                                                       self.device, "output")
        self._call("execute_block_device", pin, n, pout, C.byref(sp), L.stream_handle(stream))
        return sp.value
