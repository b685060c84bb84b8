"""In-process A/B of the spectrometer's kernels against the route it replaces (MI355X).

Per shape (M, K, D, A), complex f32 with real f32 taps, one stream of 2^log2n input samples per call:
  auto          sd.Spectrometer as it comes (automatic kernel and sub-blocks per workgroup)
  frame_rN      the per-frame kernel at N sub-blocks per workgroup (--sweep)
  slide_rN      the sliding kernel at N sub-blocks per workgroup
  oschan        sd.OversampledChannelizer alone, its [frames][M] output left in HBM: the lower bound of
                the route replaced
  oschan_torch  that call plus (y.real^2 + y.imag^2).view(S, J, A, M).sum(2): the route replaced
  copy          sdsp_bandwidth_copy_device moving the byte model's bytes (8 per input sample read,
                4 M / (32 D) of partials and 4 M / (A D) of spectra written), half read and half written
Untimed settle passes over every contestant come before each round; within a round the order is
shuffled; each call is timed with device events on one stream (one call per window: two medians whose
min .. max spreads overlap are reported as indistinguishable, not as a difference).  Every spectrometer
contestant's spectra are compared bit for bit with frame_r1's at the timed size.  One JSON document on
stdout and in --out.

    python tools/spec_ab.py --log2n 27 --rounds 5 --out profiles/r21/spec_ab.json
"""
import argparse
import json
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(M, K, D, A) for M, D in ((64, 32), (64, 64), (128, 64), (256, 128), (1024, 512), (1024, 1024))
          for K in (1, 8) for A in (32, 1024)]
TUNE_SPEC_KERNEL, TUNE_SPEC_SUBBLOCKS = 31, 32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27, help="log2 of the input samples per call")
    ap.add_argument("--rounds", type=int, default=5, help="timed rounds (shuffled), at least 3")
    ap.add_argument("--settle", type=int, default=1, help="untimed passes over every contestant before each round")
    ap.add_argument("--sweep", default="1,2,4,8", help="sub-blocks per workgroup of the frame_rN / slide_rN contestants")
    ap.add_argument("--shapes", default=None, help="only the shapes whose key contains this text")
    ap.add_argument("--seed", type=int, default=21)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert args.rounds >= 3
    sweep = [int(v) for v in args.sweep.split(",") if v]

    import torch
    import solid_dsp_amd as sd
    assert torch.cuda.is_available(), "spec_ab needs an MI355X"
    n = 1 << args.log2n
    s = torch.cuda.current_stream()
    d_in = torch.empty(n, dtype=torch.complex64, device="cuda")
    sd.lib().sdsp_synth_f32_device(d_in.data_ptr(), 20250321, 0, 0, 2 * n, None)
    d_y = torch.empty(2 * n, dtype=torch.complex64, device="cuda")  # the channeliser's frames at the largest M / D
    d_out = torch.empty(2 * n // 32, dtype=torch.float32, device="cuda")  # spectra at the largest M / (A D)
    d_ref = torch.empty_like(d_out)
    torch.cuda.synchronize()
    rng = random.Random(args.seed)
    r0 = np.random.default_rng(args.seed)
    res = {"log2_samples": args.log2n, "rounds": args.rounds, "settle": args.settle, "pair": "RC32", "shapes": {}}
    for M, K, D, A in SHAPES:
        key = f"M{M}_K{K}_D{D}_A{A}"
        if args.shapes and args.shapes not in key:
            continue
        frames = n // D
        J = frames // A
        assert n % D == 0 and frames % A == 0 and frames * M <= d_y.numel() and J * M <= d_out.numel()
        h = (r0.standard_normal(K * M) / np.sqrt(K * M)).astype(np.float32)  # white: nothing for a kernel to skip

        def spec(kernel, sub=0):
            c = sd.Spectrometer(h, M, D, A, sample_dtype=np.complex64)
            c.set_tuning(TUNE_SPEC_KERNEL, kernel)
            c.set_tuning(TUNE_SPEC_SUBBLOCKS, sub)
            return c

        handles = {"auto": spec(0)}
        for r in sweep:
            handles[f"frame_r{r}"] = spec(1, r)
            handles[f"slide_r{r}"] = spec(2, r)
        info = {k: list(c.info()) for k, c in handles.items()}
        assert all(info[f"frame_r{r}"] == [1, r] and info[f"slide_r{r}"] == [2, r] for r in sweep), info
        osc = sd.OversampledChannelizer(h, M, D, sample_dtype=np.complex64)

        def run_spec(c, out=d_out):
            assert c.execute_block_device(d_in, n, out, s) == J  # (frames % A == 0: every call starts at filled = 0)

        def oschan_torch():
            osc.execute_block_device(d_in, n, d_y, s)
            y = d_y[:frames * M]
            return (y.real ** 2 + y.imag ** 2).view(1, J, A, M).sum(2)

        runs = {k: (lambda c=c: run_spec(c)) for k, c in handles.items()}
        runs["oschan"] = lambda: osc.execute_block_device(d_in, n, d_y, s)
        runs["oschan_torch"] = oschan_torch
        model = 8 * n + 4 * frames * M // 32 + 4 * J * M
        runs["copy"] = lambda: sd.lib().sdsp_bandwidth_copy_device(d_in.data_ptr(), d_y.data_ptr(), model // 2,
                                                                   sd._lib.stream_handle(s))
        # the same bits from every spectrometer contestant (each on a fresh state, first call)
        run_spec(handles["frame_r1"], d_ref)
        same = {}
        for k, c in handles.items():
            if k != "frame_r1":
                run_spec(c)
                torch.cuda.synchronize()
                same[k] = bool(torch.equal(d_out[:J * M].view(torch.int32), d_ref[:J * M].view(torch.int32)))
        # the route replaced computes the same spectra to f32 rounding (its torch sum has another order)
        t = oschan_torch().reshape(-1).double()
        route_rel = float(((t - d_ref[:J * M].double()).norm() / t.norm()).item())
        del t
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
        best = min(handles, key=lambda k: med[k])
        slower = sorted(k for k in handles if hi[k] < lo["auto"])  # contestants faster than auto, ranges apart
        res["shapes"][key] = {
            "input_samples": n, "frames": frames, "spectra": J, "kernel_and_subblocks": info,
            "bit_identical_to_frame_r1": same, "route_replaced_rel_difference": route_rel,
            "median_ms": med, "min_ms": lo, "max_ms": hi,
            "model_bytes": model, "route_replaced_bytes": 8 * n + 2 * 8 * frames * M + 4 * J * M,
            "fraction_of_model_at_copy_rate": {k: med["copy"] / med[k] for k in handles},
            "slide_lds_bytes": (K * M + D + 3 * M) * 8,
            "fastest": best, "faster_than_auto_ranges_apart": slower,
            "oschan_over_auto": med["oschan"] / med["auto"],
            "oschan_torch_over_auto": med["oschan_torch"] / med["auto"],
            "auto_vs_oschan_distinguishable": bool(hi["auto"] < lo["oschan"] or hi["oschan"] < lo["auto"]),
        }
        print(key, {k: round(v, 3) for k, v in med.items()}, "auto", info["auto"], "faster apart:", slower,
              file=sys.stderr, flush=True)
        del handles, runs, osc
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
