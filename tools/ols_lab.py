"""Interleaved in-process A/B of overlap-save one-shot kernel variants (tools
only): loads tools/_build/libsdsp_lab.so (make -f tools/lab.mk), which carries
extra template instances of fir_ols_os_kernel selected by
sdsp_lab_set_ols_variant.  Shuffled order every round, median of rounds
(guide §5.4 rule 24), after a clock-settling phase.

  OLS_CASES="0,4,4:18432,24::2,24:::b" OLS_ROUNDS=15 python tools/ols_lab.py
A case is var[:dyn_lds_bytes[:prologue[:label]]].  prologue 2 runs the variants built with it (24,
262168, 4194328) through round 6's start-up path (the long argument list), anything else through
the product's; the label only tells two otherwise equal cases apart (an A/A).  OLS_LAB_LIB names
another build of the lab library (the parent commit's, for its A/A).  With a stamped variant
(bit 262144) and OLS_TIMELINE=DIR the workgroup timeline goes to DIR/wg_timeline.md and
DIR/wg_timeline.json (OLS_TIMELINE_TAG is appended to the names).  OLS_BURST=B times B back-to-back calls per
sample (the bench's sustained regime) instead of one isolated call.  Variant bits (kern_fir_ols_os.hip): 1
wave-level sync for the two wave-local phase boundaries; 2 no HBM traffic
(ablation); 4 HBM traffic only (ablation); 16 XCDs interleaved in runs of
`chunk` segments instead of contiguous eighths.  dyn_lds pins occupancy
(36 KB static: +18432 -> 3 workgroups per CU, +45056 -> 2).
"""
import ctypes as C
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


# the stamped points of a workgroup's wave 0 (tools/lab/ols_lab.hip sdsp_lab_ols_stamps), in time order:
# column of the s_memtime stamp, name of the interval that ends there
STAMPS = [(4, "entry -> first row load issued (start-up path)"),
          (5, "-> rows landed (row wait)"),
          (6, "-> past the P1->P2 barrier (P1: DFT16, twiddles, LDS stores, barrier wait)"),
          (7, "-> spectrum arrived, P3 products start (P2, first DFT16 of P3, spectrum wait)"),
          (8, "-> past the P4->P5 barrier (rest of P3, P4, barrier wait)"),
          (2, "-> last store issued (P5)")]


def timeline(st, ghz):
    """per-interval statistics over the sampled workgroups: s_memtime ticks are 100 MHz x
    (core clock / 100 MHz) as the entry/exit pair of memtime and realtime stamps measures it;
    cycles here are s_memtime ticks, microseconds are ticks / the run's median clock"""
    life = st[:, 2] - st[:, 0]
    rows, prev = [], st[:, 0]
    for col, name in STAMPS:
        d = st[:, col] - prev
        prev = st[:, col]
        rows.append({"interval": name, "cycles_median": float(np.median(d)), "cycles_p10": float(np.percentile(d, 10)),
                     "cycles_p90": float(np.percentile(d, 90)), "us_median": float(np.median(d)) / (ghz * 1e3),
                     "share_of_lifetime": float(np.median(d / life))})
    return {"workgroups": int(len(st)), "clock_GHz": ghz, "lifetime_cycles_median": float(np.median(life)),
            "lifetime_cycles_p10": float(np.percentile(life, 10)), "lifetime_cycles_p90": float(np.percentile(life, 90)),
            "lifetime_us_median": float(np.median(life)) / (ghz * 1e3), "intervals": rows}


def write_timeline(out_dir, tag, timelines, clocks, res, burst):
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "wg_timeline%s.json" % tag), "w") as fh:
        json.dump({"burst": burst, "timelines": timelines, "clocks": clocks, "times": res}, fh, indent=1)
    with open(os.path.join(out_dir, "wg_timeline%s.md" % tag), "w") as fh:
        fh.write("# Workgroup timeline of the one-shot overlap-save kernel (tools/ols_lab.py)\n\n"
                 "Wave 0 of every 32nd workgroup, 2^30 samples, cfg2 taps, after %d back-to-back calls; cycles are\n"
                 "s_memtime ticks.  A case is variant:dynamic LDS:prologue:label (prologue 2 = round 6's).\n" % max(burst, 20))
        for name, t in timelines.items():
            fh.write("\n## %s\n\n%d workgroups, clock %.3f GHz, lifetime median %.0f cycles (p10 %.0f, p90 %.0f) = %.2f us; "
                     "call time median %.4f ms\n\n" % (name, t["workgroups"], t["clock_GHz"], t["lifetime_cycles_median"],
                                                       t["lifetime_cycles_p10"], t["lifetime_cycles_p90"],
                                                       t["lifetime_us_median"], res[name]["median_ms"]))
            fh.write("| interval | median cycles | p10 | p90 | median us | share of lifetime |\n|---|---:|---:|---:|---:|---:|\n")
            for r in t["intervals"]:
                fh.write("| %s | %.0f | %.0f | %.0f | %.3f | %.1f %% |\n" % (
                    r["interval"], r["cycles_median"], r["cycles_p10"], r["cycles_p90"], r["us_median"],
                    100 * r["share_of_lifetime"]))
        fh.write("\n## Call times of this run (ms, median of the rounds)\n\n| case | median | min |\n|---|---:|---:|\n")
        for name, r in res.items():
            fh.write("| %s | %.4f | %.4f |\n" % (name, r["median_ms"], r["min_ms"]))


def main(rounds=int(os.environ.get("OLS_ROUNDS", "15")), log2n=30):
    import torch
    import solid_dsp_amd._lib as LL
    LL.LIB_PATH = os.environ.get("OLS_LAB_LIB") or os.path.join(REPO, "tools", "_build", "libsdsp_lab.so")
    import solid_dsp_amd as sd
    from solid_dsp_amd import FIRFilter
    from solid_dsp_amd.filter import firdes
    L = sd.lib()
    L.sdsp_lab_set_ols_variant.argtypes = [C.c_int, C.c_int, C.c_int]
    L.sdsp_lab_ols_stamps.argtypes = [C.c_void_p]
    words = L.sdsp_lab_ols_stamp_words() if hasattr(L, "sdsp_lab_ols_stamp_words") else 4
    set_variant = lambda v: L.sdsp_lab_set_ols_variant(*v[:3])  # noqa: E731
    if os.environ.get("OLS_HWID"):  # which CU slots the lab tickets use: distinct (XCC_ID, HW_ID[15:8])
        nb = 4096
        hb = torch.zeros(2 * nb, dtype=torch.int32, device="cuda")
        assert L.sdsp_lab_hwid_probe(C.c_void_p(hb.data_ptr()), nb) == 0
        a = hb.cpu().numpy().astype(np.int64).reshape(-1, 2)
        keys = set(((a[:, 0] & 7) << 8 | ((a[:, 1] >> 8) & 255)).tolist())
        print("hwid: %d distinct slots over %d blocks; xcc values %s; hw_id samples %s" % (
            len(keys), nb, sorted(set(a[:, 0].tolist()))[:16], [hex(v) for v in a[:8, 1]]), flush=True)
    n = 1 << log2n
    h = firdes.firdes_kaiser(256, 0.1, 80.0, 0.0).astype(np.float32)
    d_in = torch.empty(n, dtype=torch.complex64, device="cuda")
    L.sdsp_synth_f32_device(d_in.data_ptr(), 20250226, 0, 0, 2 * n, None)
    def parse(c):
        if c == "nco":  # the NCO mix_down of the same buffer (cfg7's kernel), for a side-by-side
            return (-1, 0, 1, "")
        f = (c.split(":") + ["", "", ""])[:4]
        return (int(f[0]), int(f[1] or 0), int(f[2] or 1), f[3])
    variants = [parse(c) for c in os.environ.get("OLS_CASES", "0,1,2,4").split(",")]
    nco = sd.NCO()
    nco.set_frequency(2 * np.pi * 0.0123)
    f = FIRFilter(h, np.float32(0.2), sample_dtype=np.complex64, algo=sd.ALGO_FFT)
    s = torch.cuda.current_stream()
    d_out = torch.empty_like(d_in)
    outs, diff = {}, {}
    for v in variants:
        if v[0] < 0 or (v[0] < 256 and v[0] & 6) or (v[0] & 131072):
            continue
        set_variant(v)
        f.reset()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        f.execute_block_device(d_in, n, d_out, s)
        e1.record(s)
        torch.cuda.synchronize()
        print("first run var%d:%d:%d:%s %.3f ms" % (v + (e0.elapsed_time(e1),)), flush=True)
        outs[v] = np.concatenate([d_out[: 1 << 22].cpu().numpy(), d_out[-(1 << 20):].cpu().numpy()])
    ref = outs.get((0, 0, 1, ""))
    for v, o in outs.items():
        diff[v] = None if ref is None else float(np.linalg.norm(o.astype(np.complex128) - ref) / np.linalg.norm(ref))
    set_variant((0, 0, 1))
    for _ in range(60):  # ~0.2 s of device time: clocks settle
        f.execute_block_device(d_in, n, d_out, s)
    torch.cuda.synchronize()
    rng = np.random.default_rng(1)
    burst = int(os.environ.get("OLS_BURST", "1"))  # > 1: back-to-back calls per sample (sustained, bench-like)
    times = {v: [] for v in variants}
    order = list(variants)
    for i in range(rounds):
        print("round", i, flush=True)
        rng.shuffle(order)
        for v in order:
            set_variant(v if v[0] >= 0 else (0, 0, 1))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(burst):
                if v[0] < 0:
                    nco.mix_block_device(d_in, n, d_out, down=True, precision=0, stream=s)
                else:
                    f.execute_block_device(d_in, n, d_out, s)
            e1.record(s)
            torch.cuda.synchronize()
            times[v].append(e0.elapsed_time(e1) / burst)
    clocks, timelines = {}, {}
    for v in variants:  # in-kernel clock of the stamped variant, after a sustained burst
        if v[0] < 0 or not (v[0] & 262144):
            continue
        set_variant(v)
        L.sdsp_lab_ols_stamps_clear()
        for _ in range(max(burst, 20)):
            f.execute_block_device(d_in, n, d_out, s)
        torch.cuda.synchronize()
        st = np.zeros(words * 8192, dtype=np.uint64)
        assert L.sdsp_lab_ols_stamps(C.c_void_p(st.ctypes.data)) == 0
        st = st.reshape(-1, words).astype(np.float64)
        ok = st[:, 3] > st[:, 1]
        ghz = (st[ok, 2] - st[ok, 0]) / (st[ok, 3] - st[ok, 1]) * 0.1
        dur_us = (st[ok, 3] - st[ok, 1]) * 0.01
        name = "var%d:%d:%d:%s" % v
        clocks[name] = {"workgroups": int(ok.sum()), "clock_GHz_median": float(np.median(ghz)),
                        "clock_GHz_p10": float(np.percentile(ghz, 10)),
                        "clock_GHz_p90": float(np.percentile(ghz, 90)),
                        "workgroup_us_median": float(np.median(dur_us))}
        if words >= 9:
            timelines[name] = timeline(st[ok], float(np.median(ghz)))
    if clocks:
        print("in-kernel clock (s_memtime / s_memrealtime x 100 MHz):", json.dumps(clocks, indent=1), flush=True)
    res = {("nco" if v[0] < 0 else "var%d:%d:%d:%s" % v): {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)),
                       "frac_of_8TBps": 16.0 * n / (np.median(t) * 1e-3) / 8e12,
                       "rel_diff_vs_var0": diff.get(v)} for v, t in times.items()}
    print(json.dumps(res, indent=1))
    if timelines and os.environ.get("OLS_TIMELINE"):
        write_timeline(os.environ["OLS_TIMELINE"], os.environ.get("OLS_TIMELINE_TAG", ""), timelines, clocks, res, burst)


if __name__ == "__main__":
    main()
