"""Times the three flat optimiser steps of csrc/train_ops.hip on one buffer of hvpr_car's parameter count: true-wd Adam
(hvpr_fused_adam_truewd_f32, 'adam_onecycle'), L2 Adam (hvpr_fused_adam_l2_f32, 'adam') and SGD at momentum 0.9
(hvpr_fused_sgd_f32, 'sgd').  Bytes per parameter: 28 for both Adam forms (p, m, v read and written, g read), 20 for SGD.

Three runs of each kernel in one process, alternating (truewd, l2, sgd, truewd, ...): a run is the median of `--iters` launches
timed one by one with device events after `--warmup` launches, with a non-null clip coefficient as in training.  The buffer size
is that of optim.FusedAdam over the model (every parameter padded to a multiple of four floats); `--numel` overrides it.  Prints
one JSON line.

    python tools/bench_optim.py [--iters 50] [--warmup 10] [--numel N]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def car_numel():
    from hvpr_amd import detector
    from hvpr_amd.config import hvpr_car_cfg
    cfg = hvpr_car_cfg()
    model = detector.build_network(cfg.MODEL, len(cfg.CLASS_NAMES), detector.SyntheticDataset(cfg, training=True))
    sizes = [p.numel() for p in model.parameters() if p.requires_grad]
    return sum((n + 3) // 4 * 4 for n in sizes), sum(sizes), len(sizes)


def main():
    import torch
    from hvpr_amd._lib import check, lib
    from hvpr_amd.kernels import _stream
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--numel", type=int, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_optim.py times GPU kernels: no GPU found")
    n, params, tensors = (args.numel, args.numel, 1) if args.numel else car_numel()
    dev = "cuda:0"
    g = torch.Generator(dev).manual_seed(20)
    p, grad = torch.randn(n, device=dev, generator=g), torch.randn(n, device=dev, generator=g) * 0.01
    m, v, buf = torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    scale = torch.tensor([0.5], device=dev)
    L, step = lib(), [0]

    def truewd():
        step[0] += 1
        check(L.hvpr_fused_adam_truewd_f32(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, 3e-4, 0.9, 0.99, 1e-8, 0.01, step[0],
                                           scale.data_ptr(), _stream()), "hvpr_fused_adam_truewd_f32")

    def l2():
        step[0] += 1
        check(L.hvpr_fused_adam_l2_f32(p.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, 3e-4, 0.9, 0.999, 1e-8, 0.01, step[0],
                                       scale.data_ptr(), _stream()), "hvpr_fused_adam_l2_f32")

    def sgd():
        check(L.hvpr_fused_sgd_f32(p.data_ptr(), grad.data_ptr(), buf.data_ptr(), n, 3e-4, 0.9, 0.01, scale.data_ptr(), _stream()),
              "hvpr_fused_sgd_f32")

    def run(fn):
        for _ in range(args.warmup):
            fn()
        times = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        return statistics.median(times)

    kernels = (("adam_truewd", truewd, 28), ("adam_l2", l2, 28), ("sgd_momentum", sgd, 20))
    runs = {name: [] for name, _, _ in kernels}
    for _ in range(3):
        for name, fn, _ in kernels:
            runs[name].append(run(fn))
    torch.cuda.synchronize()
    out = {"bench": "optim_step", "numel": n, "parameters": params, "tensors": tensors, "finite": bool(torch.isfinite(p).all())}
    for name, _, bytes_per in kernels:
        med = statistics.median(runs[name])
        out[name] = {"us_runs": [round(t, 2) for t in runs[name]], "us": round(med, 2), "bytes_per_parameter": bytes_per,
                     "GB_per_s": round(bytes_per * n / med / 1e3, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
