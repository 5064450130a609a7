"""HIP-event time of samaudio_op_noise at the benchmark's noise shape beside torch.randn of that shape, in one process
(profiles/seeded_noise/README.md).  Usage: python tools/noise_probe.py [rows frames channels rounds]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sam_audio_amd.noise import seeded_noise  # noqa: E402

HBM_WRITE_ROOF = 8.0e12   # bytes / s: the MI355X's HBM3E rate as its data sheet states it


def main():
    rows, frames, channels, rounds = (int(v) for v in (sys.argv[1:5] + ["32", "250", "256", "200"][len(sys.argv) - 1:]))
    dev = torch.device("cuda:0")
    ids = list(range(rows))
    out = torch.empty(rows, frames, channels, device=dev)
    ref = torch.empty_like(out)
    arms = {"samaudio_op_noise": lambda: seeded_noise(1234, ids, 1, frames, channels, dev, out=out),
            "torch.randn": lambda: torch.randn(rows, frames, channels, device=dev, out=ref)}
    for fn in arms.values():   # warm up: code objects, the allocator
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(rounds):   # alternating, one event pair per call
        for name, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3)
    nbytes = out.numel() * 4
    print(f"shape [{rows}, {frames}, {channels}] fp32 = {nbytes / 1e6:.3f} MB, {rounds} alternating rounds, HIP events around one call")
    for name, t in times.items():
        t.sort()
        med, lo = t[len(t) // 2], t[0]
        print(f"{name}: median {med:.2f} us, min {lo:.2f} us, {nbytes / med / 1e3:.1f} GB/s at the median = "
              f"{100 * nbytes / (med * 1e-6) / HBM_WRITE_ROOF:.1f} % of the {HBM_WRITE_ROOF / 1e12:.1f} TB/s HBM write roof")
    print(f"mean {out.mean().item():.3e}, variance {out.var().item():.5f}")


if __name__ == "__main__":
    main()
