"""General FFT: the plan shapes and the steady state that tests/test_gpu_fft.py leaves out.

Reference throughout: numpy.fft in complex128 (ifft * n for REVERSE) on seeded standard_normal
inputs.  The inputs are f32-representable, so the complex64 and the complex128 plan of one size
share one input and one reference.  Every transform of a batch is judged on its own
(gpu_util.rel_rms_rows): one misplaced bin of an N-point transform of white input is a rel-RMS
of about 1 / sqrt(N), 2.4e-4 at 2^24, far above every tolerance here.

Tolerances: test_fft_large_and_any_size's 5e-6 (c64) / 1e-12 (c128) for every length it already
asserts; longer transforms scale them by the FFT's O(eps log N) growth, log2(N) / 20 for powers
of two (2^20 is the longest four-step asserted there) and log2(M) / 18 for Bluestein at the
convolution length M (its longest there, 100003, has M = 2^18).
"""
import math

import numpy as np
import pytest

from gpu_util import bits_equal, rel_rms_rows, to_dev, to_host

pytestmark = pytest.mark.gpu

sd = pytest.importorskip("solid_dsp_amd")
from solid_dsp_amd import FFT, FFTDirection  # noqa: E402
from solid_dsp_amd import _lib as L  # noqa: E402

C64, C128 = np.complex64, np.complex128
FWD, REV = FFTDirection.FORWARD, FFTDirection.REVERSE
TOL = {C64: 5e-6, C128: 1e-12}
PRECS = [C64, C128]


class _Case:
    """Seeded [batch, n] input (f32-representable) and its complex128 references."""

    def __init__(self, n, batch):
        rng = np.random.default_rng(1000003 * batch + n)
        self.n, self.batch = n, batch
        self.x = np.empty((batch, n), C64)
        self.x.real = rng.standard_normal((batch, n), dtype=np.float32)
        self.x.imag = rng.standard_normal((batch, n), dtype=np.float32)
        self._ref = {}

    def ref(self, d):
        if d not in self._ref:
            xs = self.x.astype(C128)
            self._ref[d] = np.fft.fft(xs, axis=-1) if d == FWD else np.fft.ifft(xs, axis=-1) * self.n
        return self._ref[d]


_last = None


def case(n, batch):
    """One case at a time stays in memory: consecutive tests of one shape share its reference."""
    global _last
    if _last is None or (_last.n, _last.batch) != (n, batch):
        _last = None
        _last = _Case(n, batch)
    return _last


def check(y, ref, tol, what):
    """Every transform within tol of its reference; prints the worst for the record."""
    r = rel_rms_rows(np.asarray(y).reshape(ref.shape), ref)
    b = int(np.argmax(r))
    print(f"{what}: max rel-RMS {r[b]:.3e} (transform {b} of {len(r)}), tol {tol:.3e}")
    assert np.all(np.isfinite(r)) and r[b] <= tol, f"{what}: transform {b} of {len(r)} rel-RMS {r[b]:.3e} > {tol:.3e}"
    return float(r[b])


# ---- A. steady state of the pipelined 1024-point pass --------------------------------------
N20 = 1 << 20
GROUPS = N20 // 1024 // 16  # 16-transform groups of one pass of one 2^20-point transform


def steady_batch():
    """Smallest batch at which every persistent workgroup of fft1024_pipe_kernel (one per CU)
    walks at least two groups, and some three, in each pass."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    batch = -(-(2 * cus + GROUPS) // GROUPS)
    assert GROUPS * batch >= 2 * cus + GROUPS, (cus, batch)
    return batch


@pytest.mark.parametrize("d", [FWD, REV])
def test_pipe_pass_steady_state(d):
    """2^20 points c64 at a batch that gives each persistent workgroup two or three groups: the
    prefetch of the next group's loads across the FFT and the stores, the LDS reuse barrier at
    the loop end and the empty-descriptor tail all run.  Out of place, in place and from an
    input 8 bytes past 16-byte alignment (8-byte instead of 16-byte lanes on the column pass)
    against numpy; the three bit-identical; and transforms of the batch bit-identical to
    batch-1 runs of the same input (where each workgroup runs one group only), because a
    group's arithmetic and twiddles depend on its own first column alone."""
    import torch
    B = steady_batch()
    c = case(N20, B)
    ref = c.ref(d)
    f = FFT(N20, d, precision=C64)
    assert f.method == "four-step"
    st = torch.cuda.current_stream()
    a = to_dev(c.x.reshape(-1))
    assert a.data_ptr() % 16 == 0
    ya = torch.empty_like(a)
    f.execute_device(a, ya, B, st)
    m = torch.empty(B * N20 + 1, dtype=torch.complex64, device="cuda")[1:]
    assert m.data_ptr() % 16 == 8
    m.copy_(a)
    ym = torch.empty_like(a)
    f.execute_device(m, ym, B, st)
    t = a.clone()
    f.execute_device(t, t, B, st)
    singles = {}
    for b in sorted({0, B // 2, B - 1}):
        singles[b] = torch.empty(N20, dtype=torch.complex64, device="cuda")
        f.execute_device(a[b * N20:(b + 1) * N20], singles[b], 1, st)
    ya, ym, t = to_host(ya), to_host(ym), to_host(t)
    check(ya, ref, TOL[C64], f"2^20 x {B} c64 {d.name} out of place")
    check(ym, ref, TOL[C64], f"2^20 x {B} c64 {d.name} misaligned input")
    check(t, ref, TOL[C64], f"2^20 x {B} c64 {d.name} in place")
    assert bits_equal(ya, ym), "aligned and misaligned inputs differ"
    assert bits_equal(ya, t), "in place and out of place differ"
    for b, y1 in singles.items():
        assert bits_equal(ya[b * N20:(b + 1) * N20], to_host(y1)), f"transform {b} of {B} differs from its batch-1 run"


@pytest.mark.parametrize("wave", [1, 8, 0])
def test_one_shot_and_generic_passes_at_the_steady_state_batch(wave):
    """the same batch through the one-shot wave kernels (16 and 8 transforms per workgroup) and
    the generic pass"""
    B = steady_batch()
    c = case(N20, B)
    f = FFT(N20, FWD, precision=C64)
    f.set_tuning(L.TUNE_FFT_WAVE1024, wave)
    check(f.execute(c.x), c.ref(FWD), TOL[C64], f"2^20 x {B} c64 FORWARD WAVE1024={wave}")


# ---- B. every four-step split ---------------------------------------------------------------
def pow2_tol(k, prec):
    return TOL[prec] * max(k, 20) / 20


def split_dirs(k):
    return (FWD, REV) if k <= 22 else (FWD,)


def split_batch(k):
    return 2 if k <= 21 else 1  # a pass crosses a transform boundary


@pytest.mark.parametrize("k,prec", [(k, p) for k in (14, 15, 17, 18, 19, 21, 22, 23, 24) for p in PRECS])
def test_four_step_every_split(k, prec):
    """N = 2^l1 * 2^l2, l1 = k / 2: 7+7 .. 12+12.  2^19 runs only its second pass on the wave
    kernel (c64, G = So = 512); 2^21 has a 1024-point first pass that the wave kernel must
    decline (its inter-pass twiddle table is 2^20's); 2^22 .. 2^24 are the 2048- and 4096-point
    generic passes (128 KB of LDS)."""
    n, batch = 1 << k, split_batch(k)
    c = case(n, batch)
    x = c.x.astype(prec)
    for d in split_dirs(k):
        f = FFT(n, d, precision=prec)
        assert f.method == "four-step"
        check(f.execute(x), c.ref(d), pow2_tol(k, prec), f"2^{k} x {batch} {np.dtype(prec).name} {d.name}")


@pytest.mark.parametrize("k,wave", [(k, w) for k in (19, 21) for w in (16, 1, 8, 0)])
def test_four_step_split_pass_variants(k, wave):
    n, batch = 1 << k, split_batch(k)
    c = case(n, batch)
    for d in split_dirs(k):
        f = FFT(n, d, precision=C64)
        f.set_tuning(L.TUNE_FFT_WAVE1024, wave)
        check(f.execute(c.x), c.ref(d), pow2_tol(k, C64), f"2^{k} x {batch} c64 {d.name} WAVE1024={wave}")


# ---- C. Bluestein over the wave passes ------------------------------------------------------
@pytest.mark.parametrize("n,prec", [(n, p) for n in (131073, 200001, 262145, 300000) for p in PRECS])
def test_bluestein_on_wave_passes(n, prec):
    """Convolution lengths 2^19 and 2^20: in c64 the 1024-point wave passes run in place on
    the work buffer, forward then inverse."""
    import torch
    M = 1 << (2 * n - 2).bit_length()
    assert M >= 2 * n - 1 > M // 2 and M in (1 << 19, 1 << 20)
    tol = TOL[prec] * math.log2(M) / 18
    c = case(n, 2)
    x = c.x.astype(prec)
    for d in (FWD, REV):
        f = FFT(n, d, precision=prec)
        assert f.method == "Bluestein"
        what = f"Bluestein {n} (M = 2^{M.bit_length() - 1}) x 2 {np.dtype(prec).name} {d.name}"
        check(f.execute(x), c.ref(d), tol, what)
        t = to_dev(x.reshape(-1))
        f.execute_device(t, t, 2, torch.cuda.current_stream())
        check(to_host(t), c.ref(d), tol, what + " in place")


# ---- D. batched small transforms ------------------------------------------------------------
@pytest.mark.parametrize("n,prec", [(n, p) for n in (1, 2, 4, 8, 64, 512, 1024, 4096) for p in PRECS])
def test_lds_fft_ragged_last_workgroup(n, prec):
    """fft_pow2_kernel packs tpb transforms into a workgroup: two full workgroups and a last
    one that holds a single transform"""
    tpb = 1 if n >= 1024 else 256 // max(n // 4, 1)
    batch = 2 * tpb + 1
    c = case(n, batch)
    x = c.x.astype(prec)
    for d in (FWD, REV):
        f = FFT(n, d, precision=prec)
        assert f.method == "Stockham (LDS)"
        check(f.execute(x), c.ref(d), TOL[prec], f"{n} x {batch} {np.dtype(prec).name} {d.name}")


@pytest.mark.parametrize("n,batch,prec", [(n, b, p) for n, b in ((3, 65536 + 3), (511, 5)) for p in PRECS])
def test_direct_dft_batches(n, batch, prec):
    """dft_direct_kernel at a batch beyond a grid's 65535-row second dimension, and at the
    largest direct size with bins in two workgroups; in place runs from a copy of the input"""
    import torch
    c = case(n, batch)
    x = c.x.astype(prec)
    for d in (FWD, REV):
        f = FFT(n, d, precision=prec)
        assert f.method == "direct DFT"
        what = f"direct DFT {n} x {batch} {np.dtype(prec).name} {d.name}"
        check(f.execute(x), c.ref(d), TOL[prec], what)
        t = to_dev(x.reshape(-1))
        f.execute_device(t, t, batch, torch.cuda.current_stream())
        check(to_host(t), c.ref(d), TOL[prec], what + " in place")


# ---- E. size limits -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2 ** 23 + 1, 2 ** 24 + 1])
@pytest.mark.parametrize("prec", PRECS)
def test_sizes_without_a_plan_are_refused(n, prec):
    """A size above 2^23 that is no power of two would convolve at 2^25 = 2^12 * 2^13, a pass
    longer than the 4096 points the pass kernels hold: refused at creation (2^24 itself plans,
    test_four_step_every_split)."""
    for d in (FWD, REV):
        with pytest.raises(sd.SdspError) as e:
            FFT(n, d, precision=prec)
        assert e.value.code == 90, e.value  # SDSP_E_INVALID_ARGUMENT
        assert "2^2" in str(e.value), e.value  # carries a message naming the limit
