"""One handle through mixed-algorithm streams: SDSP_ALGO_AUTO picks the kernel per call from the
block length, and sdsp_*_set_algo may change it between two blocks of a running stream, so the
state (delay line or section state, ping-pong buffer, decimation phase, host window) crosses
from one kernel to the other on every such call.

Oracle of the stream tests (run_fir_schedule, run_iir_schedule), for a handle A under test:
  1. per call: a fresh handle pinned to the algorithm the call must resolve to, restored with
     A's state, given the same block the same way, must give A's output and A's next state bit
     for bit; FIR states are also the last L-1 inputs bit for bit;
  2. an unobserved twin of A (no get_state between calls) gives A's concatenated output bits;
  3. against the CPU restatement: reference-order FIR / decimator calls are bit-equal to the f32
     restatement at their positions; the whole output meets the project's criteria against the
     f64 restatement (FIR / decimator: section 8d at 1e-6, rel-RMS and max|err| <= 1e-6 sum|h|
     max|x|; IIR: rel-RMS <= tol and max|err| <= tol max|ref|, tol 1e-5 for f32 coefficients and
     1e-12 for f64), and the max-abs clause holds on its own over the first 2L (IIR: 512)
     outputs of every call, reported with the call index.

Which side ran is read from the library: sdsp_fir_get_algo, sdsp_fir_device_ops (predicted per
call from the documented coherence rule: one read-back before the first host step after device
work, one upload before the first device call after host steps), wscan_mode(), and bit equality
with the pinned handle of that algorithm (at a threshold length, also inequality with the other
one)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from gpu_util import bits_equal, rel_rms, to_dev, empty_dev, to_host

pytestmark = pytest.mark.gpu

sd = pytest.importorskip("solid_dsp_amd")
from solid_dsp_amd import (FIRFilter, DecimatingFIRFilter, PolyPhaseFilterBank, InterpolatingFIRFilter,  # noqa: E402
                           IIRFilter, DecimatingIIRFilter, InterpolatingIIRFilter, IIRFilterType)

C64, C128, F32, F64 = np.complex64, np.complex128, np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SEED = 20251020
FIR_LONG = 1 << 16   # AUTO: FIR / decimator blocks of at least this many samples take the fast kernel
IIR_LONG = 1 << 13   # AUTO: IIR blocks of at least this many samples (n * interpolation) take the scan
HOST_MACS = 1 << 16  # host blocks of n * L up to this many multiply-adds run on the host delay line
SO, NORMAL = IIRFilterType.SecondOrder, IIRFilterType.Normal
ALGO_NAME = {sd.ALGO_AUTO: "AUTO", sd.ALGO_EXACT: "EXACT", sd.ALGO_FMA: "FMA", sd.ALGO_FFT: "FFT"}


@pytest.fixture
def default_auto():
    old = sd.get_default_algo()
    sd.set_default_algo(sd.ALGO_AUTO)
    try:
        yield
    finally:
        sd.set_default_algo(old)


def _frozen(a):
    a.setflags(write=False)
    return a


def _is_c(dt):
    return np.dtype(dt).kind == "c"


def _wide(a):
    return np.asarray(a).astype(C128 if _is_c(np.asarray(a).dtype) else F64)


@functools.lru_cache(maxsize=None)
def stream(ch, n, complex_=True):
    return _frozen(O.synth(SEED, ch, 0, n, complex_=complex_))


@functools.lru_cache(maxsize=None)
def fir_taps(dt, L, fc=0.1):
    """real low-pass taps (RR32 / RC32), or the same shifted off centre: complex taps (CC32)"""
    h = O.firdes_kaiser(L, fc, 80.0, 0.0)
    if dt == O.CC32:
        return _frozen((h * np.exp(2j * np.pi * 0.07 * np.arange(L))).astype(C64))
    return _frozen(h.astype(F32))


def fir_scale(dt):
    return C64(0.2 + 0.1j) if dt == O.CC32 else F32(0.2)


WIDE_DT = {O.RR32: O.RR64, O.RC32: O.RC64, O.CC32: O.CC64}


def fir_max_bound(h, x, tol=1e-6):
    return tol * float(np.sum(np.abs(np.asarray(h, dtype=C128)))) * float(np.max(np.abs(np.asarray(x, dtype=C128))))


def assert_fir_tol(y, ref, h, x, tol):
    """section 8d, both criteria (as test_gpu_fir.assert_fir_tol): rel_RMS <= tol and
    max|err| <= tol * sum|h| * max|x|, h the scaled taps"""
    y = np.asarray(y, dtype=C128)
    ref = np.asarray(ref, dtype=C128)
    assert y.shape == ref.shape
    assert rel_rms(y, ref) <= tol, rel_rms(y, ref)
    bound = fir_max_bound(h, x, tol)
    err = float(np.max(np.abs(y - ref))) if y.size else 0.0
    assert err <= bound, (err, bound)


# ---------------------------------------------------------------- schedules
# A schedule is a list of (op, n) over consecutive samples of one stream:
#   "s" n per-sample execute calls      "p" n push calls (decimator)      "w" one write of n samples
#   "h" one execute_block on a host slice                  "d" one execute_block_device on a device slice
FIR_SCHEDULE = [
    ("s", 3),       # 0  host steps on the zeroed window
    ("h", 200),     # 1  host block, n * L <= 65536: host delay line
    ("h", 4096),    # 2  host -> reference-order kernel (upload), window fed from the host slice
    ("s", 2),       # 3  reference-order kernel -> host on the fed window (no read-back)
    ("h", 65536),   # 4  host -> overlap-save (upload), host block at the threshold
    ("s", 4),       # 5  overlap-save -> host on the fed window
    ("d", 70001),   # 6  long block directly after per-sample calls (upload); 8 bytes past 16-byte alignment
    ("s", 4),       # 7  per-sample calls directly after a long device block (read-back)
    ("d", 1000),    # 8  host -> reference-order kernel, device block
    ("d", 65536),   # 9  reference-order -> overlap-save at the threshold, 16-byte aligned slice
    ("d", 1),       # 10 a block of length 1 directly after a long block: overlap-save -> reference order
    ("h", 65535),   # 11 one below the threshold: reference order
    ("h", 65536),   # 12 reference order -> overlap-save
    ("h", 1),       # 13 a host block of length 1 directly after a long block: overlap-save -> host (read-back)
    ("h", 4096),    # 14 host -> reference-order kernel, window fed
    ("s", 2),       # 15 and the fed window read by the host again
]
DECIM_SCHEDULE = [
    ("s", 3),       # 0  host steps, the phase moves
    ("h", 200),     # 1  host block on the host delay line
    ("p", 5),       # 2  push: the phase moves without output
    ("d", 65536),   # 3  host -> FMA polyphase kernel at the threshold, starting at a non-zero phase
    ("w", 13),      # 4  write on the host (read-back)
    ("h", 65535),   # 5  one below the threshold: reference order (upload), window fed
    ("w", 300),     # 6  write as device work (n * L > 65536), window fed
    ("s", 2),       # 7  host steps on the fed window
    ("d", 70001),   # 8  long block, length no multiple of M, non-zero phase
    ("p", 3),       # 9  push directly after a long device block (read-back)
    ("h", 65536),   # 10 host block at the threshold: FMA
    ("d", 4097),    # 11 FMA -> reference order on the device
    ("d", 65536),   # 12 reference order -> FMA
    ("s", 4),       # 13 FMA -> host
]
IIR_SCHEDULE = [1, 100, 8191, 8192, 37, 70001, 8191, 20000]
IIR_SCHEDULE_INTERP3 = [1, 100, 2730, 2731, 37, 70001, 2730, 20000]  # the threshold is on n * 3


def schedule_len(schedule):
    return sum(n for _, n in schedule)


def host_side(op, n, L):
    return op in "sp" or (op in "hw" and n * L <= HOST_MACS)


def fir_resolved(op, n, L, decim):
    """what ALGO_AUTO must resolve to for this call of a 32-bit complex FIR / decimating handle"""
    if host_side(op, n, L) or n < FIR_LONG:
        return sd.ALGO_EXACT
    return sd.ALGO_FMA if decim else sd.ALGO_FFT


class OpsModel:
    """sdsp_fir_device_ops over a schedule, from the coherence rule of the host step: a host-side
    call costs one read-back if the host does not hold the window, else nothing; device work
    costs one upload if host steps ran since, plus the launch; a device-resident input drops the
    host window, a host input moves it on"""

    def __init__(self):
        self.host_valid, self.dev_stale = True, False

    def step(self, op, n, L):
        if host_side(op, n, L):
            d = 0 if self.host_valid else 1
            self.host_valid, self.dev_stale = True, True
            return d
        d = 1 + (1 if self.dev_stale else 0)
        self.dev_stale = False
        if op == "d":
            self.host_valid = False
        return d


def run_call(f, op, seg, dev=None):
    """one schedule entry on handle f; dev = (device input slice, device output slice) for "d" """
    sdt = f.sample_dtype
    if op == "s":
        out = [v for s in seg for v in f.execute(s)]
        return np.array(out, dtype=sdt)
    if op == "p":
        for s in seg:
            f.push(s)
        return np.zeros(0, dtype=sdt)
    if op == "w":
        f.write(seg)
        return np.zeros(0, dtype=sdt)
    if op == "h":
        return f.execute_block(seg)
    import torch
    d_in, d_out = dev
    got = f.execute_block_device(d_in, len(seg), d_out, torch.cuda.current_stream())
    return to_host(d_out)[:got].copy()


def restatement_calls(make, schedule, x):
    """the CPU restatement through a schedule: the outputs of every entry"""
    o = make()
    outs, off = [], 0
    for op, n in schedule:
        seg = x[off:off + n]
        if op == "p":
            for v in seg:
                o.push(v)
            outs.append(np.zeros(0, dtype=o.in_dt))
        elif op == "w":
            o.write(seg)
            outs.append(np.zeros(0, dtype=o.in_dt))
        else:
            outs.append(o.execute_block(seg))
        off += n
    return outs


def device_ops(f):
    return int(sd.lib().sdsp_fir_device_ops(f._h))


def get_algo(f):
    return int(sd.lib().sdsp_fir_get_algo(f._h))


def check_handoff_windows(y, ref, starts, width, bound, what):
    """the max-abs clause on its own over the first `width` outputs from every call start"""
    y, ref = np.asarray(y, dtype=C128), np.asarray(ref, dtype=C128)
    for k, s in enumerate(starts):
        if s >= len(y):
            continue
        err = float(np.abs(y[s:s + width] - ref[s:s + width]).max())
        assert err <= bound, f"{what}: call {k}: max|err| {err:.3e} > {bound:.3e} over outputs [{s}, {s + width})"


def run_fir_schedule(make, pinned, schedule, x, L, M, resolve, ref32_calls, ref64_calls, hs, expect_algo=None,
                     model_ops=True, set_algo=None):
    """oracle steps 1-3 for a FIR / decimating FIR handle.
    make() -> the handle under test; pinned(algo) -> a fresh handle pinned to algo;
    resolve(k, op, n) -> the algorithm call k must run; set_algo[k] -> algorithm set before call k;
    hs = the scaled taps of the section 8d bound"""
    n_total = schedule_len(schedule)
    assert len(x) >= n_total
    A = make()
    d_x = to_dev(np.array(x[:n_total]))  # a writable copy: the cached stream is read-only
    d_outs = [empty_dev(n_total, x.dtype) for _ in range(3)]
    assert d_x.data_ptr() % 16 == 0 and all(d.data_ptr() % 16 == 0 for d in d_outs)
    xpad = np.concatenate([np.zeros(L - 1, dtype=x.dtype), x[:n_total]])
    model = OpsModel()
    ys, starts, algos = [], [], []
    off = ooff = 0
    for k, (op, n) in enumerate(schedule):
        what = f"call {k} {op}{n}"
        if set_algo is not None:
            A.set_algo(set_algo[k])
        if expect_algo is not None:
            assert get_algo(A) == expect_algo, what
        algo = resolve(k, op, n)
        seg = x[off:off + n]
        state, phase = A.get_state()
        assert phase == off % M, what
        B = pinned(algo)
        B.set_state(state, phase)
        nout = A.output_count(n)
        if op not in "pw":
            assert nout == B.output_count(n) == len(ref32_calls[k]), what
        devA = devB = None
        if op == "d":
            devA = (d_x[off:off + n], d_outs[0][ooff:ooff + max(nout, 1)])
            devB = (d_x[off:off + n], d_outs[1][ooff:ooff + max(nout, 1)])
        ops0 = device_ops(A)
        yA = run_call(A, op, seg, devA)
        dops = device_ops(A) - ops0
        yB = run_call(B, op, seg, devB)
        assert len(yA) == len(ref32_calls[k]) == len(ref64_calls[k]), (what, len(yA), len(ref32_calls[k]))
        assert bits_equal(yA, yB), f"{what}: differs from a fresh {ALGO_NAME[algo]} handle restored with the state"
        if model_ops:
            want = model.step(op, n, L)
            assert dops == want, f"{what}: device_ops moved by {dops}, expected {want}"
            assert host_side(op, n, L) or dops >= 1, what
        stA, phA = A.get_state()
        stB, phB = B.get_state()
        assert phA == phB == (off + n) % M, what
        assert bits_equal(stA, stB), f"{what}: state differs from the pinned handle's"
        assert bits_equal(stA, xpad[off + n:off + n + L - 1]), f"{what}: state is not the last L-1 inputs"
        if algo == sd.ALGO_EXACT:
            assert bits_equal(yA, ref32_calls[k]), f"{what}: reference-order call differs from the f32 restatement"
        elif n in (FIR_LONG, FIR_LONG + 1) or set_algo is not None:
            # the fast kernel is a different computation: a handle pinned to the reference order,
            # restored with the same state, gives other bits (so the equality above tells them apart)
            E = pinned(sd.ALGO_EXACT)
            E.set_state(state, phase)
            devE = (devA[0], d_outs[2][ooff:ooff + max(nout, 1)]) if op == "d" else None
            assert not bits_equal(yA, run_call(E, op, seg, devE)), f"{what}: same bits as the reference order"
        ys.append(yA)
        starts.append(ooff)
        algos.append(algo)
        off += n
        ooff += len(yA)
    y = np.concatenate(ys)
    T = make()
    off = ooff = 0
    yt = []
    for k, (op, n) in enumerate(schedule):
        if set_algo is not None:
            T.set_algo(set_algo[k])
        nout = T.output_count(n)
        dev = (d_x[off:off + n], d_outs[1][ooff:ooff + max(nout, 1)]) if op == "d" else None
        yt.append(run_call(T, op, x[off:off + n], dev))
        off += n
        ooff += len(yt[-1])
    assert bits_equal(np.concatenate(yt), y), "the unobserved twin differs: a state read hides a missing flush or pull"
    assert device_ops(T) == device_ops(A), "get_state moved device_ops"
    ref64 = np.concatenate(ref64_calls)
    check_handoff_windows(y, ref64, starts, 2 * L, fir_max_bound(hs, x[:n_total]), "8d max-abs after a handoff")
    assert_fir_tol(y, ref64, hs, x[:n_total], 1e-6)
    return y, algos


# ---------------------------------------------------------------- 1. FIR under AUTO
@functools.lru_cache(maxsize=None)
def fir_refs(dt, L, n):
    h, s, x = fir_taps(dt, L), fir_scale(dt), stream(1, n)
    ref32 = _frozen(O.fir(dt, h, s).execute_block(x))
    ref64 = _frozen(O.fir(WIDE_DT[dt], _wide(h), _wide(s)[()]).execute_block(_wide(x)))
    return ref32, ref64


def split_calls(a, schedule):
    out, off = [], 0
    for _, n in schedule:
        out.append(a[off:off + n])
        off += n
    return out


def test_fir_schedule_alignment_and_sides():
    """the schedule itself: the 70001 block starts 8 bytes past 16-byte alignment, the 65536 device
    block on it; the lengths sit on the intended side of both thresholds for L = 64 and 300"""
    off, at = 0, {}
    for k, (op, n) in enumerate(FIR_SCHEDULE):
        at[k] = off
        off += n
    assert FIR_SCHEDULE[6] == ("d", 70001) and at[6] % 2 == 1
    assert FIR_SCHEDULE[9] == ("d", 65536) and at[9] % 2 == 0
    for L in (64, 300):
        assert host_side("h", 200, L) and not host_side("h", 4096, L)
        assert host_side("h", 1, L) and not host_side("d", 1, L)
    for M in (32, 7):
        off = 0
        for k, (op, n) in enumerate(DECIM_SCHEDULE):
            if k in (3, 8):
                assert op == "d" and off % M != 0 and n >= FIR_LONG
            off += n
        assert 70001 % M != 0
    assert 300 * 256 > HOST_MACS and 13 * 300 <= HOST_MACS


@pytest.mark.parametrize("L", [64, 300])
@pytest.mark.parametrize("dt", [O.RC32, O.CC32])
def test_auto_fir_one_handle_mixed_blocks(default_auto, dt, L):
    """per-sample calls, host-run blocks, host blocks on the device and device-resident blocks on
    both sides of 65535 / 65536 through one AUTO handle with the host step on (L = 300: two halo
    rows, no multiple of 256)"""
    n = schedule_len(FIR_SCHEDULE)
    h, s, x = fir_taps(dt, L), fir_scale(dt), stream(1, n)
    ref32, ref64 = fir_refs(dt, L, n)

    def make():
        return FIRFilter(h, s, sample_dtype=C64)  # no algo: the process default, AUTO

    def pinned(algo):
        return FIRFilter(h, s, sample_dtype=C64, algo=algo)

    y, algos = run_fir_schedule(make, pinned, FIR_SCHEDULE, x, L, 1, lambda k, op, m: fir_resolved(op, m, L, False),
                                split_calls(ref32, FIR_SCHEDULE), split_calls(ref64, FIR_SCHEDULE),
                                _wide(h) * _wide(s)[()], expect_algo=sd.ALGO_AUTO)
    want = [sd.ALGO_FFT if k in (4, 6, 9, 12) else sd.ALGO_EXACT for k in range(len(FIR_SCHEDULE))]
    assert algos == want


def test_auto_fir_clone_after_host_steps(default_auto):
    """clone while the host window is newer than the device history: the clone starts from the
    flushed window, keeps AUTO, and takes the same kernels as the original on both sides"""
    dt, L = O.RC32, 300
    n0, n1, n2 = 105, 105 + FIR_LONG, 105 + FIR_LONG + 3
    h, s, x = fir_taps(dt, L), fir_scale(dt), stream(1, n2)
    ref32 = O.fir(dt, h, s).execute_block(x)
    a = FIRFilter(h, s, sample_dtype=C64)
    y0 = np.concatenate([run_call(a, "s", x[:5]), a.execute_block(x[5:n0])])
    assert bits_equal(y0, ref32[:n0])
    c = a.clone()
    assert get_algo(c) == get_algo(a) == sd.ALGO_AUTO
    p = FIRFilter(h, s, sample_dtype=C64, algo=sd.ALGO_FFT)
    p.set_state(np.concatenate([np.zeros(L - 1 - n0, dtype=C64), x[:n0]]))
    ya, yc, yp = a.execute_block(x[n0:n1]), c.execute_block(x[n0:n1]), p.execute_block(x[n0:n1])
    assert bits_equal(ya, yp) and bits_equal(yc, yp)  # overlap-save from the same history
    assert not bits_equal(ya, ref32[n0:n1])
    for f in (a, c):  # back on the host steps (the clone reads its window back from the device)
        assert bits_equal(run_call(f, "s", x[n1:n2]), ref32[n1:n2])
        assert bits_equal(f.get_state()[0], x[n2 - (L - 1):n2])


# ---------------------------------------------------------------- 2. decimating FIR under AUTO
@functools.lru_cache(maxsize=None)
def decim_case(L, M):
    h = _frozen(O.firdes_kaiser(L, 0.5 / M, 80.0, 0.0).astype(F32))
    s = F32(1.0 / M)
    x = stream(2, schedule_len(DECIM_SCHEDULE))
    r32 = restatement_calls(lambda: O.decim(O.RC32, h, s, M), DECIM_SCHEDULE, x)
    r64 = restatement_calls(lambda: O.decim(O.RC64, h.astype(F64), F64(s), M), DECIM_SCHEDULE, x.astype(C128))
    return h, s, x, [_frozen(r) for r in r32], [_frozen(r) for r in r64]


@pytest.mark.parametrize("L,M", [(256, 32), (300, 7)])
def test_auto_decim_one_handle_mixed_blocks(default_auto, L, M):
    """cfg4 shape (256 taps, M = 32: the column-parallel polyphase kernel) and 300 taps, M = 7 (the
    tiled fallback): push / write phase moves between blocks, 65535 / 65536 inputs, long blocks
    that start at a non-zero phase and whose length is no multiple of M; the output count of
    every call is the restatement's"""
    h, s, x, r32, r64 = decim_case(L, M)

    def make():
        return DecimatingFIRFilter(h, s, M, sample_dtype=C64)

    def pinned(algo):
        return DecimatingFIRFilter(h, s, M, sample_dtype=C64, algo=algo)

    y, algos = run_fir_schedule(make, pinned, DECIM_SCHEDULE, x, L, M,
                                lambda k, op, m: fir_resolved(op, m, L, True), r32, r64, h.astype(F64) * F64(s),
                                expect_algo=sd.ALGO_AUTO)
    want = [sd.ALGO_FMA if k in (3, 8, 10, 12) else sd.ALGO_EXACT for k in range(len(DECIM_SCHEDULE))]
    assert algos == want


def test_auto_decim_f64_stays_reference_order(default_auto):
    """RC64: AUTO keeps a 64-bit handle on the reference order at every length"""
    L, M, n = 256, 32, 70001
    h = O.firdes_kaiser(L, 0.5 / M, 80.0, 0.0)
    x = stream(3, n).astype(C128)
    d = DecimatingFIRFilter(h, 1.0 / M, M, sample_dtype=C128)
    assert get_algo(d) == sd.ALGO_AUTO
    o = O.decim(O.RC64, h, 1.0 / M, M)
    for a, b in [(0, 5), (5, n)]:  # 5 inputs on the host step, then 69996 >= 65536 on the device
        assert bits_equal(d.execute_block(x[a:b]), o.execute_block(x[a:b])), (a, b)
    d2 = DecimatingFIRFilter(h, 1.0 / M, M, sample_dtype=C128)
    assert bits_equal(d2.execute_block(x), O.decim(O.RC64, h, 1.0 / M, M).execute_block(x))


# ---------------------------------------------------------------- 3. IIR under AUTO
def butter():
    sos = np.array(json.load(open(os.path.join(HERE, "golden", "butter8_0p2_sos.json")))["sos"])
    return sos[:, :3].reshape(-1), sos[:, 3:].reshape(-1)


def normal4():
    """an order-4 direct-form pair: two sections of the butter-8 cascade multiplied out
    (pole radii 0.59 and 0.71), unit gain at DC"""
    ff, fb = butter()
    b = np.convolve(ff[3:6], ff[6:9])
    a = np.convolve(fb[3:6], fb[6:9])
    return b * (a.sum() / b.sum()), a


IIR_CASES = {  # name: (type, coefficient dtype, sample dtype, restatement dtype, f64 restatement dtype)
    "sos_rr32": (SO, F32, F32, O.RR32, O.RR64),
    "sos_rc32": (SO, F32, C64, O.RC32, O.RC64),
    "sos_rr64": (SO, F64, F64, O.RR64, O.RR64),
    "normal4_rr32": (NORMAL, F32, F32, O.RR32, O.RR64),
}
IIR_MODES = {"plain": (0, 1), "decim5": (1, 5), "interp3": (2, 3)}


def iir_make(case, mode, algo=None):
    type_, cdt, sdt, _, _ = IIR_CASES[case]
    ff, fb = normal4() if type_ == NORMAL else butter()
    ff, fb = ff.astype(cdt), fb.astype(cdt)
    kind, M = IIR_MODES[mode]
    kw = dict(sample_dtype=sdt)
    if algo is not None:
        kw["algo"] = algo
    if kind == 0:
        return IIRFilter(ff, fb, type_, **kw)
    if kind == 1:
        return DecimatingIIRFilter(ff, fb, type_, M, **kw)
    return InterpolatingIIRFilter(ff, fb, type_, M, **kw)


@functools.lru_cache(maxsize=None)
def iir_ref64(case, mode, n):
    type_, cdt, sdt, _, wdt = IIR_CASES[case]
    ff, fb = normal4() if type_ == NORMAL else butter()
    ff, fb = ff.astype(cdt).astype(F64), fb.astype(cdt).astype(F64)
    kind, M = IIR_MODES[mode]
    t = O.NORMAL if type_ == NORMAL else O.SECOND_ORDER
    o = O.iir(wdt, ff, fb, t) if kind == 0 else (O.iir_decim if kind == 1 else O.iir_interp)(wdt, ff, fb, t, M)
    x = stream(4, n, complex_=_is_c(sdt))
    return _frozen(o.execute_block(_wide(x)))


def iir_tol(cdt):
    return 1e-5 if cdt == F32 else 1e-12


def run_iir_schedule(case, mode, lengths, algo_of_call, set_algo=None, make=None):
    """oracle steps 1-3 for an IIR handle: host blocks of `lengths`; algo_of_call(k, nd) is the
    algorithm call k must run (nd = n * interpolation)"""
    type_, cdt, sdt, _, _ = IIR_CASES[case]
    kind, M = IIR_MODES[mode]
    Mi = M if kind == 2 else 1
    n_total = sum(lengths)
    x = stream(4, n_total, complex_=_is_c(sdt)).astype(sdt)
    ref = iir_ref64(case, mode, n_total)
    A = make() if make else iir_make(case, mode)
    assert A.wscan_mode() != 0, "the cascade admits no wave scan: the long calls would stay serial"
    ys, starts, algos = [], [], []
    off = ooff = 0
    for k, n in enumerate(lengths):
        what = f"{case} {mode} call {k} n={n}"
        if set_algo is not None:
            A.set_algo(set_algo[k])
        algo = algo_of_call(k, n * Mi)
        state, phase = A.get_state()
        assert phase == (off % M if kind == 1 else 0), what
        B = iir_make(case, mode, algo=algo)
        B.set_state(state, phase)
        seg = x[off:off + n]
        yA, yB = A.execute_block(seg), B.execute_block(seg)
        assert bits_equal(yA, yB), f"{what}: differs from a fresh {ALGO_NAME[algo]} handle restored with the state"
        stA, phA = A.get_state()
        stB, phB = B.get_state()
        assert phA == phB and bits_equal(stA, stB), f"{what}: state differs from the pinned handle's"
        if IIR_LONG - Mi <= n * Mi < IIR_LONG + Mi or set_algo is not None:
            # at the threshold the two kernels are told apart: the other one gives other bits
            other = sd.ALGO_EXACT if algo == sd.ALGO_FMA else sd.ALGO_FMA
            X = iir_make(case, mode, algo=other)
            X.set_state(state, phase)
            assert not bits_equal(yA, X.execute_block(seg)), f"{what}: same bits as {ALGO_NAME[other]}"
        ys.append(yA)
        starts.append(ooff)
        algos.append(algo)
        off += n
        ooff += len(yA)
    y = np.concatenate(ys)
    T = make() if make else iir_make(case, mode)
    off = 0
    yt = []
    for k, n in enumerate(lengths):
        if set_algo is not None:
            T.set_algo(set_algo[k])
        yt.append(T.execute_block(x[off:off + n]))
        off += n
    assert bits_equal(np.concatenate(yt), y), "the unobserved twin differs"
    tol = iir_tol(cdt)
    assert y.shape == ref.shape
    bound = tol * float(np.abs(ref).max())
    check_handoff_windows(y, ref, starts, 512, bound, f"{case} {mode}: max-abs after a handoff")
    assert rel_rms(y, ref) <= tol, rel_rms(y, ref)
    assert float(np.abs(_wide(y) - ref).max()) <= bound
    return algos


@pytest.mark.parametrize("mode", list(IIR_MODES))
@pytest.mark.parametrize("case", list(IIR_CASES))
def test_auto_iir_one_handle_serial_and_scan(default_auto, case, mode):
    """serial -> scan -> serial through one AUTO handle on both sides of 8191 / 8192 (n * M for
    the interpolator: 2730 serial, 2731 scan): the section state crosses between the serial
    recurrence's coordinates and the scan's"""
    lengths = IIR_SCHEDULE_INTERP3 if mode == "interp3" else IIR_SCHEDULE
    algos = run_iir_schedule(case, mode, lengths,
                             lambda k, nd: sd.ALGO_FMA if nd >= IIR_LONG else sd.ALGO_EXACT)
    E, S = sd.ALGO_EXACT, sd.ALGO_FMA
    assert algos == [E, E, E, S, E, S, E, S]


# ---------------------------------------------------------------- 4. set_algo between blocks
SET_ALGO_BLOCK = 20001


@pytest.mark.parametrize("dt", [O.RC32, O.RR32])
def test_set_algo_between_blocks_fir(dt):
    """EXACT -> FFT -> FMA -> FFT -> EXACT -> AUTO before blocks of 20001 samples, every call device
    work (host_step=False); RR32 is the packed-pair overlap-save kernel"""
    L = 300
    seq = [sd.ALGO_EXACT, sd.ALGO_FFT, sd.ALGO_FMA, sd.ALGO_FFT, sd.ALGO_EXACT, sd.ALGO_AUTO]
    schedule = [("h", SET_ALGO_BLOCK)] * len(seq)
    n = schedule_len(schedule)
    sdt = C64 if dt == O.RC32 else F32
    h, s = fir_taps(dt, L), F32(0.2)
    x = stream(5, n, complex_=dt == O.RC32)
    ref32 = O.fir(dt, h, s).execute_block(x)
    ref64 = O.fir(WIDE_DT[dt], h.astype(F64), F64(s)).execute_block(_wide(x))

    def make():
        return FIRFilter(h, s, sample_dtype=sdt, host_step=False, algo=sd.ALGO_EXACT)

    def pinned(algo):
        return FIRFilter(h, s, sample_dtype=sdt, host_step=False, algo=algo)

    # 20001 < 65536: AUTO resolves to the reference order
    resolve = lambda k, op, m: sd.ALGO_EXACT if seq[k] == sd.ALGO_AUTO else seq[k]  # noqa: E731
    run_fir_schedule(make, pinned, schedule, x, L, 1, resolve, split_calls(ref32, schedule),
                     split_calls(ref64, schedule), h.astype(F64) * F64(s), model_ops=False, set_algo=seq)


def test_set_algo_between_blocks_iir():
    """EXACT -> FMA -> EXACT -> AUTO -> FMA on an RR32 butter-8 cascade (20001 >= 8192: AUTO scans)"""
    seq = [sd.ALGO_EXACT, sd.ALGO_FMA, sd.ALGO_EXACT, sd.ALGO_AUTO, sd.ALGO_FMA]
    algos = run_iir_schedule("sos_rr32", "plain", [SET_ALGO_BLOCK] * len(seq),
                             lambda k, nd: sd.ALGO_FMA if seq[k] == sd.ALGO_AUTO else seq[k], set_algo=seq,
                             make=lambda: iir_make("sos_rr32", "plain", algo=sd.ALGO_EXACT))
    assert algos == [sd.ALGO_EXACT, sd.ALGO_FMA, sd.ALGO_EXACT, sd.ALGO_FMA, sd.ALGO_FMA]


def test_set_algo_fft_refused_mid_stream_leaves_the_stream_alone():
    """set_algo(ALGO_FFT) on a decimating handle and on an f64 handle fails with Unsupported (91)
    between two blocks; algorithm, state and the rest of the stream are untouched"""
    L, n, cut = 256, 40000, 20001
    h32 = fir_taps(O.RC32, L)
    cases = [
        (DecimatingFIRFilter(h32, F32(0.2), 2, sample_dtype=C64, host_step=False),
         O.decim(O.RC32, h32, F32(0.2), 2), stream(6, n)),
        (FIRFilter(h32.astype(F64), 0.2, sample_dtype=C128, host_step=False),
         O.fir(O.RC64, h32.astype(F64), 0.2), stream(6, n).astype(C128)),
    ]
    for f, o, x in cases:
        before = get_algo(f)
        assert bits_equal(f.execute_block(x[:cut]), o.execute_block(x[:cut]))
        state, phase = f.get_state()
        with pytest.raises(sd.SdspError) as e:
            f.set_algo(sd.ALGO_FFT)
        assert e.value.code == 91
        assert get_algo(f) == before
        state2, phase2 = f.get_state()
        assert phase2 == phase and bits_equal(state2, state)
        assert bits_equal(f.execute_block(x[cut:]), o.execute_block(x[cut:]))


# ---------------------------------------------------------------- 5. handle edits after the plan exists
TUNE_OLS_KERNEL, OLS_ONESHOT_WIDE = 14, 3


def test_ols_plan_survives_handle_edits():
    """CC32, ALGO_FFT, L = 300: set_scale to another complex scale, clone, set_channels(3) and reset
    after the overlap-save plan was built by a first block"""
    dt, L = O.CC32, 300
    h = fir_taps(dt, L)
    s0, s1 = C64(0.2 + 0.1j), C64(-0.3 + 0.25j)
    n1, n2, n3 = 30001, 60002, 90003
    x = stream(7, n3)
    h64 = h.astype(C128)

    def tuned(scale, channels=1):
        g = FIRFilter(h, scale, sample_dtype=C64, algo=sd.ALGO_FFT, channels=channels)
        g.set_tuning(TUNE_OLS_KERNEL, OLS_ONESHOT_WIDE)
        return g

    def ref64(scale, xs):
        return O.fir(O.CC64, h64, C128(scale)).execute_block(xs.astype(C128))

    f = tuned(s0)
    # 1. the plan exists
    y1 = f.execute_block(x[:n1])
    assert_fir_tol(y1, ref64(s0, x[:n1]), h64 * C128(s0), x[:n1], 1e-6)
    # 2. another complex scale: the tables are rebuilt, the history carried
    f.set_scale(s1)
    assert f.get_scale() == s1
    y2 = f.execute_block(x[n1:n2])
    assert_fir_tol(y2, ref64(s1, x[:n2])[n1:], h64 * C128(s1), x[:n2], 1e-6)
    # 3. clone: same algorithm (and kernel choice), the original's bits on the next block
    c = f.clone()
    assert get_algo(c) == get_algo(f) == sd.ALGO_FFT
    assert c.get_scale() == s1
    y3, y3c = f.execute_block(x[n2:n3]), c.execute_block(x[n2:n3])
    assert bits_equal(y3, y3c)
    assert_fir_tol(y3, ref64(s1, x[:n3])[n2:], h64 * C128(s1), x[:n3], 1e-6)
    g = tuned(s1)  # a fresh handle given the history computes the same bits: nothing else was carried
    g.set_state(x[n2 - (L - 1):n2])
    assert bits_equal(y3, g.execute_block(x[n2:n3]))
    # 4. three channels (the state is cleared): an odd block (rows off 16-byte alignment), an even one
    f.set_channels(3)
    assert get_algo(f) == sd.ALGO_FFT
    state, _ = f.get_state()
    assert len(state) == 3 * (L - 1) and not state.any()
    fresh = tuned(s1, channels=3)
    xs = np.stack([stream(10 + c_, 50003) for c_ in range(3)])
    cuts = [0, 20001, 50003]
    ys = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        blk = np.ascontiguousarray(xs[:, a:b])
        ys.append(f.execute_block(blk))
        assert bits_equal(ys[-1], fresh.execute_block(blk)), (a, b)
        st, _ = f.get_state()
        assert bits_equal(st, np.ascontiguousarray(xs[:, b - (L - 1):b]).reshape(-1)), (a, b)
    y = np.concatenate(ys, axis=-1)
    for c_ in range(3):
        assert_fir_tol(y[c_], ref64(s1, xs[c_]), h64 * C128(s1), xs[c_], 1e-6)
    # 5. reset: a fresh handle's bits
    f.reset()
    blk = np.ascontiguousarray(xs[:, :30000])
    assert bits_equal(f.execute_block(blk), tuned(s1, channels=3).execute_block(blk))


# ---------------------------------------------------------------- 6. PFB / interpolator under a default of AUTO
def test_default_auto_leaves_pfb_and_interp_exact(default_auto):
    """PFB and interpolator handles know EXACT and FMA only: with the process default at AUTO they
    stay on the reference order, at any block length"""
    assert sd.get_default_algo() == sd.ALGO_AUTO
    probe = FIRFilter(fir_taps(O.RC32, 64), F32(0.2), sample_dtype=C64)
    assert get_algo(probe) == sd.ALGO_AUTO  # the default is live: FIR handles do start on AUTO
    hp = fir_taps(O.RC32, 64, 1.0 / 16)
    x = stream(8, 70000)
    p = PolyPhaseFilterBank(hp, 8, F32(0.5), sample_dtype=C64)
    assert bits_equal(p.execute_block(x), O.pfb(O.RC32, hp, 8, F32(0.5)).execute_block(x))
    hi = fir_taps(O.RC32, 256, 1.0 / 64)
    i = InterpolatingFIRFilter(hi, 32, sample_dtype=C64)  # the tiled shape
    assert bits_equal(i.execute_block(x[:3001]), O.interp(O.RC32, hi, 32).execute_block(x[:3001]))


# ---------------------------------------------------------------- 7. the environment variable
_CHILD = r"""
import json, sys
import numpy as np
import solid_dsp_amd as sd
from solid_dsp_amd import FIRFilter, DecimatingFIRFilter, IIRFilter, IIRFilterType
F32, C64 = np.float32, np.complex64
rng = np.random.default_rng(7)
n = 1 << 16
x = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(C64)
xr = rng.standard_normal(n).astype(F32)
h = (np.hanning(256) * np.sinc(0.2 * (np.arange(256) - 127.5))).astype(F32)
sos = np.array(json.load(open(sys.argv[1]))["sos"])
b, a = sos[:, :3].reshape(-1).astype(F32), sos[:, 3:].reshape(-1).astype(F32)
SO = IIRFilterType.SecondOrder
eq = lambda u, v: u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes()
fir = lambda **k: FIRFilter(h, F32(0.2), sample_dtype=C64, host_step=False, **k)
dec = lambda **k: DecimatingFIRFilter(h, F32(1.0 / 32), 32, sample_dtype=C64, host_step=False, **k)
iir = lambda **k: IIRFilter(b, a, SO, sample_dtype=F32, **k)
ga = sd.lib().sdsp_fir_get_algo
f, d, i = fir(), dec(), iir()
res = {"default": sd.get_default_algo(), "fir_algo": ga(f._h), "decim_algo": ga(d._h), "iir_wscan": i.wscan_mode() != 0}
for name, mk, fast, xs in (("fir", fir, sd.ALGO_FFT, x), ("decim", dec, sd.ALGO_FMA, x), ("iir", iir, sd.ALGO_FMA, xr)):
    yl = mk().execute_block(xs)
    res[name + "_long_fast"] = bool(eq(yl, mk(algo=fast).execute_block(xs)))
    res[name + "_long_exact"] = bool(eq(yl, mk(algo=sd.ALGO_EXACT).execute_block(xs)))
    ys = mk().execute_block(xs[:4096])
    res[name + "_short_exact"] = bool(eq(ys, mk(algo=sd.ALGO_EXACT).execute_block(xs[:4096])))
    res[name + "_short_fast"] = bool(eq(ys, mk(algo=fast).execute_block(xs[:4096])))
print("RESULT " + json.dumps(res, sort_keys=True))
"""


def test_env_default_auto_reaches_device_handles():
    """SDSP_DEFAULT_ALGO=auto in a fresh child process: handles built with no algo argument report
    AUTO, run a 65536-sample block on the fast kernels and a 4096-sample block on the reference
    order (the IIR handle has no algorithm query: it is read from which kernel's bits it gives)"""
    env = dict(os.environ)
    env["SDSP_DEFAULT_ALGO"] = "auto"
    out = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(HERE, "golden", "butter8_0p2_sos.json")],
                         cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(lines) == 1, out.stdout[-2000:]
    res = json.loads(lines[0][len("RESULT "):])
    want = {"default": sd.ALGO_AUTO, "fir_algo": sd.ALGO_AUTO, "decim_algo": sd.ALGO_AUTO, "iir_wscan": True}
    for name in ("fir", "decim", "iir"):
        want.update({name + "_long_fast": True, name + "_long_exact": False,
                     name + "_short_exact": True, name + "_short_fast": False})
    assert res == want, res
    assert sd.get_default_algo() == sd.ALGO_EXACT  # this process is untouched
