"""In-process A/B of the rational resampler's kernels against the interpolator alone (MI355X).

Per shape (M, D, K), on a c32 stream with real f32 taps (RC32), ALGO_FMA:
  interp   the InterpolatingFIRFilter alone on the same input: the cheapest first stage a caller
           has without the resampler (it still has to pick every D-th sample afterwards)
  auto     sd.Resampler on its automatic selection
  staged / per_output / branch   sd.Resampler forced to each kernel that applies to the shape
  copy     sdsp_bandwidth_copy_device over the resampler's own byte count, so each time can be
           read against the byte model: 8 B written + 8 D / M B read per output
Untimed settle passes over every contestant come before each round; within a round the order is
shuffled; each call is timed with device events on one stream (one call per window: a ratio
inside the recorded min .. max spread of its two medians is reported as indistinguishable, not as
a difference).  The outputs of every forced kernel are compared bit for bit with the automatic
one's at the timed size.  One JSON document on stdout and in --out.

    python tools/resamp_ab.py --log2n 30 --rounds 6 --out profiles/r14/resamp_ab.json
"""
import argparse
import json
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(3, 2, 16), (2, 3, 16), (5, 4, 8), (25, 24, 8), (147, 160, 16), (8, 2, 8), (1, 4, 16)]  # (M, D, K)
NAMES = {1: "staged", 2: "per_output", 3: "branch"}
TUNE_RESAMP_KERNEL = 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=30, help="log2 of the interpolator's outputs per call (n * M)")
    ap.add_argument("--rounds", type=int, default=6, help="timed rounds (alternating, shuffled), at least 3")
    ap.add_argument("--settle", type=int, default=1, help="untimed passes over every contestant before each round")
    ap.add_argument("--seed", type=int, default=14)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 3

    import torch
    import solid_dsp_amd as sd
    assert torch.cuda.is_available(), "resamp_ab needs an MI355X"
    total = 1 << args.log2n
    s = torch.cuda.current_stream()
    d_in = torch.empty(total, dtype=torch.complex64, device="cuda")  # M = 1 reads all of it
    sd.lib().sdsp_synth_f32_device(d_in.data_ptr(), 20250226, 0, 0, 2 * total, None)
    mid = torch.empty(total + 256, dtype=torch.complex64, device="cuda")  # the interpolator's output
    torch.cuda.synchronize()
    rng = random.Random(args.seed)
    r0 = np.random.default_rng(args.seed)
    res = {"log2_interp_outputs": args.log2n, "rounds": args.rounds, "settle": args.settle, "algo": "FMA",
           "pair": "RC32", "shapes": {}}
    for M, D, K in SHAPES:
        n = total // M
        L = K * M
        h = (r0.standard_normal(L) / np.sqrt(L)).astype(np.float32)  # white: nothing for a kernel to skip
        itp = sd.InterpolatingFIRFilter(h, M, sample_dtype=np.complex64, algo=sd.ALGO_FMA)
        probe = sd.Resampler(h, M, D, sample_dtype=np.complex64, algo=sd.ALGO_FMA)
        nout = probe.output_count(n)
        handles, kernel = {"auto": probe}, {"auto": NAMES[probe.info()[0]]}
        for k, name in NAMES.items():
            r = sd.Resampler(h, M, D, sample_dtype=np.complex64, algo=sd.ALGO_FMA)
            r.set_tuning(TUNE_RESAMP_KERNEL, k)
            if r.info()[0] == k:  # else the kernel does not apply to the shape
                handles[name] = r
                kernel[name] = name
        outs = {name: torch.empty(nout + 1, dtype=torch.complex64, device="cuda") for name in handles}
        bytes_model = 8 * nout + 8 * n
        cp_a = torch.empty(bytes_model // 2 // 16 * 16, dtype=torch.uint8, device="cuda")
        cp_b = torch.empty_like(cp_a)

        def run_resamp(name):  # (phase and window carry over: n_out moves by at most one between calls)
            handles[name].execute_block_device(d_in, n, outs[name], s)

        def run_interp():
            itp.execute_block_device(d_in, n, mid, s)

        def run_copy():  # reads half the model's bytes and writes half
            sd.lib().sdsp_bandwidth_copy_device(cp_a.data_ptr(), cp_b.data_ptr(), cp_a.numel(), sd._lib.stream_handle(s))

        runs = {name: (lambda name=name: run_resamp(name)) for name in handles}
        runs["interp"] = run_interp
        runs["copy"] = run_copy
        for name in handles:
            run_resamp(name)
        torch.cuda.synchronize()
        same = {name: bool(torch.equal(torch.view_as_real(outs[name][:nout]).view(torch.int32),
                                       torch.view_as_real(outs["auto"][:nout]).view(torch.int32)))
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
        res["shapes"][f"M{M}_D{D}_K{K}"] = {
            "inputs": n, "outputs": nout, "kernel": kernel, "tile": {k: handles[k].info()[1] for k in handles},
            "forced_vs_auto_bit_identical": same,
            "median_ms": med, "min_ms": lo, "max_ms": hi,
            "model_bytes": bytes_model,
            "interp_bytes": 8 * n * M + 8 * n,
            "copy_GBps": copy_gbps,
            "model_ms_at_copy_rate": bytes_model / (copy_gbps * 1e9) * 1e3,
            "over_interp": {k: med[k] / med["interp"] for k in handles},
            "auto_slower_than_interp": bool(D >= 2 and med["auto"] > med["interp"]),
            "auto_interp_distinguishable": bool(hi["auto"] < lo["interp"] or hi["interp"] < lo["auto"]),
        }
        del itp, probe, handles, outs, cp_a, cp_b
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
