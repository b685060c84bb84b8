"""In-process A/B of the arbitrary-rate resampler's kernels against the route it replaces (MI355X).

Per shape (K, rate), on a c32 stream with real f32 taps (RC32), P = 64 branches, ALGO_FMA, n inputs:
  staged / per_output   sd.ArbResampler forced to each kernel that applies to the shape
  auto       sd.ArbResampler on its automatic selection
  copy       sdsp_bandwidth_copy_device over the resampler's algorithmic bytes (n inputs read,
             n_out outputs written), so each time can be read against the byte model
  resamp     sd.Resampler at 147/160 with the same K on the same input, for context
  interp     the route this replaces: the InterpolatingFIRFilter by P writing all n P samples (a
             caller would then read two neighbours per output back).  Run as --interp-chunks calls
             over consecutive parts of the input into one buffer of n P / chunks samples, timed as
             one window: the same bytes to HBM without an allocation of 8 n P bytes
Untimed settle passes over every contestant come before each round; within a round the order is
shuffled; each contestant is timed with device events on one stream (a ratio inside the recorded
min .. max spread of its two medians is reported as indistinguishable, not as a difference).  The
outputs of both kernels are compared bit for bit at the timed size.  One JSON document on stdout
and in --out.

    python tools/arb_ab.py --log2n 26 --rounds 6 --out profiles/r19/arb_ab.json
"""
import argparse
import json
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

P = 64
SHAPES = [(8, 0.9187512345), (8, 2.718281828), (16, 0.9187512345), (16, 2.718281828)]  # (K, rate)
NAMES = {1: "staged", 2: "per_output"}
TUNE_ARB_KERNEL = 29
PEAK_BPS = 8e12  # HBM3E peak of the MI355X the fractions are quoted against


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=26, help="log2 of the inputs per call")
    ap.add_argument("--rounds", type=int, default=6, help="timed rounds (alternating, shuffled), at least 3")
    ap.add_argument("--settle", type=int, default=1, help="untimed passes over every contestant before each round")
    ap.add_argument("--interp-chunks", type=int, default=16, help="calls the interpolate-by-P route is split into")
    ap.add_argument("--seed", type=int, default=19)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 3

    import torch
    import solid_dsp_amd as sd
    assert torch.cuda.is_available(), "arb_ab needs an MI355X"
    n = 1 << args.log2n
    chunks = args.interp_chunks
    assert n % chunks == 0
    s = torch.cuda.current_stream()
    d_in = torch.empty(n, dtype=torch.complex64, device="cuda")
    sd.lib().sdsp_synth_f32_device(d_in.data_ptr(), 20250226, 0, 0, 2 * n, None)
    mid = torch.empty(n // chunks * P + 256, dtype=torch.complex64, device="cuda")  # the interpolator's output
    torch.cuda.synchronize()
    rng = random.Random(args.seed)
    r0 = np.random.default_rng(args.seed)
    res = {"log2_inputs": args.log2n, "rounds": args.rounds, "settle": args.settle, "algo": "FMA", "pair": "RC32",
           "filters": P, "interp_chunks": chunks, "shapes": {}}
    for K, rate in SHAPES:
        L = K * P
        h = (r0.standard_normal(L) / np.sqrt(L)).astype(np.float32)  # white: nothing for a kernel to skip
        itp = sd.InterpolatingFIRFilter(h, P, sample_dtype=np.complex64, algo=sd.ALGO_FMA)
        h147 = (r0.standard_normal(K * 147) / np.sqrt(K * 147)).astype(np.float32)
        rat = sd.Resampler(h147, 147, 160, sample_dtype=np.complex64, algo=sd.ALGO_FMA)
        probe = sd.ArbResampler(h, P, rate=rate, sample_dtype=np.complex64, algo=sd.ALGO_FMA)
        nout = probe.output_count(n) + 1  # (t carries over: n_out moves by at most one between calls)
        handles, kernel = {"auto": probe}, {"auto": NAMES[probe.info()[0]]}
        for k, name in NAMES.items():
            r = sd.ArbResampler(h, P, rate=rate, sample_dtype=np.complex64, algo=sd.ALGO_FMA)
            r.set_tuning(TUNE_ARB_KERNEL, k)
            if r.info()[0] == k:  # else the kernel does not apply to the shape
                handles[name] = r
                kernel[name] = name
        outs = {name: torch.empty(nout + 1, dtype=torch.complex64, device="cuda") for name in handles}
        out_rat = torch.empty(rat.output_count(n) + 2, dtype=torch.complex64, device="cuda")
        bytes_model = 8 * (nout - 1) + 8 * n
        cp_a = torch.empty(bytes_model // 2 // 16 * 16, dtype=torch.uint8, device="cuda")
        cp_b = torch.empty_like(cp_a)

        def run_arb(name):
            handles[name].execute_block_device(d_in, n, outs[name], s)

        def run_interp():
            for c in range(chunks):
                itp.execute_block_device(d_in[c * (n // chunks):], n // chunks, mid, s)

        def run_resamp():
            rat.execute_block_device(d_in, n, out_rat, s)

        def run_copy():  # reads half the model's bytes and writes half
            sd.lib().sdsp_bandwidth_copy_device(cp_a.data_ptr(), cp_b.data_ptr(), cp_a.numel(), sd._lib.stream_handle(s))

        runs = {name: (lambda name=name: run_arb(name)) for name in handles}
        runs["interp"] = run_interp
        runs["resamp"] = run_resamp
        runs["copy"] = run_copy
        for name in handles:  # every handle from t = 0 on the same window: the same outputs
            run_arb(name)
        torch.cuda.synchronize()
        first = nout - 1
        same = {name: bool(torch.equal(torch.view_as_real(outs[name][:first]).view(torch.int32),
                                       torch.view_as_real(outs["auto"][:first]).view(torch.int32)))
                for name in handles if name != "auto"}
        times = {k: [] for k in runs}
        for _ in range(args.rounds):
            for _ in range(args.settle):
                for f in runs.values():
                    f()
            torch.cuda.synchronize()
            order = list(runs)
            rng.shuffle(order)
            for k in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                runs[k]()
                e1.record(s)
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1))
        med = {k: float(np.median(v)) for k, v in times.items()}
        lo = {k: float(np.min(v)) for k, v in times.items()}
        hi = {k: float(np.max(v)) for k, v in times.items()}
        copy_gbps = 2 * cp_a.numel() / (med["copy"] * 1e-3) / 1e9
        best = min(handles, key=lambda k: med[k])
        res["shapes"][f"K{K}_rate{rate}"] = {
            "inputs": n, "outputs": first, "step": probe.step(), "kernel": kernel,
            "tile": {k: handles[k].info()[1] for k in handles},
            "forced_vs_auto_bit_identical": same,
            "median_ms": med, "min_ms": lo, "max_ms": hi,
            "model_bytes": bytes_model,
            "interp_bytes": 8 * n * P + 8 * n,
            "copy_GBps": copy_gbps,
            "model_ms_at_copy_rate": bytes_model / (copy_gbps * 1e9) * 1e3,
            "fraction_of_8TBps": {k: bytes_model / (med[k] * 1e-3) / PEAK_BPS for k in handles},
            "over_interp": {k: med[k] / med["interp"] for k in handles},
            "over_copy": {k: med[k] / med["copy"] for k in handles},
            "staged_beats_interp": bool("staged" in handles and hi["staged"] < lo["interp"]),
            "staged_per_output_distinguishable": bool("staged" in handles and (
                hi["staged"] < lo["per_output"] or hi["per_output"] < lo["staged"])),
            "fastest": best,
        }
        del itp, rat, probe, handles, outs, out_rat, cp_a, cp_b
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
