#!/usr/bin/env python
"""The sound-activity ranker on one batch of candidates: the HIP kernels against the reference's path, which
copies every candidate to the host and runs pydub's silence detection there (its CPU statement, tests/activity_ref.py).
usage: python tools/activity_probe.py [clips] [candidates] [seconds] [rate] [reps]     (default 8 x 8 x 10 s at 48 000 Hz, 20 rounds)
       python tools/activity_probe.py kernels [clips] [candidates] [seconds] [rate]    (the launches only, for a kernel trace)

  kernels    the `clips` samaudio_op_activity calls (two launches each) between device events, workspace and outputs allocated before
  forward    SoundActivityRanker.forward end to end: the span upload, the allocations, the launches; device events, and the host clock
             to a device synchronise
  cpu        the waveforms copied to the host (timed), then tests/activity_ref.py's statement and score per candidate, one thread
and the ranker's scores against the statement's, which must be equal.  One span per clip."""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sam_audio_amd import activity, hip  # noqa: E402
from sam_audio_amd.ranking import SoundActivityRanker  # noqa: E402
from tests import activity_ref as A  # noqa: E402

argv = sys.argv[1:]
only_kernels = argv[:1] == ["kernels"]
if only_kernels:
    argv = argv[1:]
n_clips, n_cand, seconds, rate = (int(argv[i]) if len(argv) > i else d for i, d in enumerate((8, 8, 10, 48000)))
reps = int(argv[4]) if len(argv) > 4 else 20
HBM_PEAK = 8.0e12
dev = torch.device("cuda:0")
samples = seconds * rate

# every candidate: noise at 1e-4 plus bursts of a 440 Hz tone at its own places
rng = np.random.default_rng(0)
t = np.arange(samples) / rate
host = np.empty((n_clips, n_cand, samples), dtype=np.float32)
for b in range(n_clips):
    for c in range(n_cand):
        x = 1e-4 * rng.uniform(-1, 1, samples)
        for start in rng.uniform(0, seconds - 1.0, 4):
            x += np.where((t >= start) & (t < start + rng.uniform(0.05, 0.9)), 0.5 * np.sin(2 * np.pi * 440 * t), 0.0)
        host[b, c] = x
wavs = torch.from_numpy(host).to(dev)
anchors = [[("+", 0.2 * seconds, 0.6 * seconds)] for _ in range(n_clips)]
candidates = [wavs[b] for b in range(n_clips)]
ranker = SoundActivityRanker()

# the launches alone
lib = hip.lib()
step, phases = activity.ratio(rate)
L = lib.samaudio_activity_length_ms(samples, step, phases)
need = lib.samaudio_activity_workspace_bytes(n_cand, samples, step, phases)
table = activity.device_table(-40, "rel_to_max", dev)
ref = torch.tensor([[a[0][1], a[0][2]] for a in anchors], dtype=torch.float64, device=dev)
work = torch.empty(need // 8, dtype=torch.int64, device=dev)
scores = torch.empty(n_clips, n_cand, device=dev)
stream = hip.current_stream_ptr()


def launches():
    for b in range(n_clips):
        hip.check(lib.samaudio_op_activity(C.c_void_p(wavs[b].data_ptr()), n_cand, samples, samples, step, phases, hip.ptr(table),
                                           C.c_void_p(ref[b].data_ptr()), 1, 0, hip.ptr(work), need, C.c_void_p(scores[b].data_ptr()),
                                           None, 0, None, None, stream))


def events(fn, n):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


read = wavs.numel() * 4
print(f"{n_clips} clips x {n_cand} candidates x {seconds} s at {rate} Hz (L = {L} ms, {read / 1e6:.1f} MB of fp32 waveforms, "
      f"{n_clips * n_cand * L * 8 / 1e6:.2f} MB of cells), one span per clip; {reps} rounds after a warm-up")
ms = events(launches, reps)
k_med = statistics.median(ms)
print(f"  kernels, {n_clips} samaudio_op_activity calls = {2 * n_clips} launches (device events): median {k_med * 1e3:.1f} us, "
      f"min {min(ms) * 1e3:.1f}, max {max(ms) * 1e3:.1f}; the waveforms once over that time: {read / (k_med * 1e-3) / 1e9:.0f} GB/s = "
      f"{read / (k_med * 1e-3) / HBM_PEAK:.3f} of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak (both kernels and the gaps between launches)")
if only_kernels:
    sys.exit(0)


def forward():
    return ranker(extracted_audio=candidates, spans=anchors, sample_rate=rate)


ms = events(forward, reps)
wall = []
for _ in range(reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = forward()
    torch.cuda.synchronize()
    wall.append((time.perf_counter() - t0) * 1e3)
print(f"  SoundActivityRanker.forward -> [{n_clips}, {n_cand}] (device events): median {statistics.median(ms) * 1e3:.1f} us, "
      f"min {min(ms) * 1e3:.1f}, max {max(ms) * 1e3:.1f}; host clock to a synchronise: median {statistics.median(wall) * 1e3:.1f} us")

# the reference's path: every candidate to the host, silence detection there
cpu_reps = max(1, min(3, reps))
copy_ms, stmt_ms = [], []
for _ in range(cpu_reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    on_host = [w.to(torch.float32).cpu() for w in candidates]
    t1 = time.perf_counter()
    want = [[float(A.score(c.numpy(), rate, [(s, e) for _, s, e in spans])) for c in clip] for clip, spans in zip(on_host, anchors)]
    t2 = time.perf_counter()
    copy_ms.append((t1 - t0) * 1e3)
    stmt_ms.append((t2 - t1) * 1e3)
c_med, s_med = statistics.median(copy_ms), statistics.median(stmt_ms)
print(f"  CPU statement on the same waveforms ({cpu_reps} rounds, one thread): copy to the host {c_med:.1f} ms + silence detection and "
      f"scores {s_med:.1f} ms = {c_med + s_med:.1f} ms")
equal = torch.equal(got.cpu(), torch.tensor(want))
print(f"  scores equal to the statement's float32: {equal}; distinct scores per clip: {[len(set(r)) for r in want]}")
sys.exit(0 if equal else 1)
