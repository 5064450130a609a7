#!/usr/bin/env python
"""The audio front end on one batch: SAMAudioProcessor with audio_transform="torch" (float64 conv1d resampler, mean and padding on the
CPU) against audio_transform="hip" (resample_mix_kernel, one launch per clip) - DESIGN.md section 10.5.
usage: python tools/audio_frontend_probe.py [clips] [seconds] [rate] [reps]            (default 32 stereo 16-bit clips of 10 s at 44 100 Hz)
       python tools/audio_frontend_probe.py memory <torch|hip|all> <files|tensors|all> [clips] [seconds] [rate]

Default: the same clips as 16-bit WAV files and as fp32 (2, samples) tensors with sampling_rates; `reps` rounds alternating the two
transforms after a warm-up, host clock around a call that ends in a device synchronise -
  __call__                  the processor alone ("torch" leaves the batch on the CPU, "hip" leaves Batch.audios on the device)
  __call__ + .to(device)    the batch where separate() wants it, both ways
  kernel                    the 32 launches alone between device events, the clips already uploaded as int16 frames
and `hip` against `torch` on the batch.  Then (`memory all all`: only) one fresh child process per (transform, input kind) in `memory`
form: the largest resident set a sampling thread sees during one call (/proc/self/statm every millisecond) over the resident set
before it, and torch.cuda.max_memory_allocated around the call."""
import os
import statistics
import subprocess
import sys
import tempfile
import threading
import time
import wave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from sam_audio_amd import SAMAudioProcessor, audio, preset_config  # noqa: E402

argv = sys.argv[1:]
memory = argv[:1] == ["memory"]
if memory:
    transform, kind, argv = argv[1], argv[2], argv[3:]
n_clips, seconds, rate = (int(argv[i]) if len(argv) > i else d for i, d in enumerate((32, 10, 44100)))
reps = int(argv[3]) if len(argv) > 3 else 7
dev = torch.device("cuda:0")
cfg = preset_config("large*")
model_rate = cfg.audio_codec.sample_rate
samples = seconds * rate


def make_clips(tmp):
    g = torch.Generator().manual_seed(1)
    pcm = [torch.randint(-32768, 32768, (2, samples), generator=g, dtype=torch.int16) for _ in range(n_clips)]
    paths = []
    for i, x in enumerate(pcm):
        paths.append(os.path.join(tmp, f"clip{i}.wav"))
        with wave.open(paths[-1], "wb") as f:
            f.setnchannels(2)
            f.setsampwidth(2)
            f.setframerate(rate)
            f.writeframes(x.t().contiguous().numpy().astype("<i2").tobytes())
    return pcm, paths, [x.float() / 32768.0 for x in pcm]


def call(proc, kind, paths, tensors, move=False):
    kw = dict(audios=paths) if kind == "files" else dict(audios=tensors, sampling_rates=[rate] * n_clips)
    batch = proc(descriptions=[""] * n_clips, **kw)
    if move:
        batch = batch.to(dev)
    torch.cuda.synchronize()
    return batch


def memory_children():
    for t in ("torch", "hip"):
        for kind in ("files", "tensors"):
            subprocess.run([sys.executable, os.path.abspath(__file__), "memory", t, kind, str(n_clips), str(seconds), str(rate)],
                           check=True, timeout=300)


if memory and transform == "all":
    memory_children()
    sys.exit(0)


def resident() -> int:
    with open("/proc/self/statm") as f:
        return int(f.read().split()[1]) * os.sysconf("SC_PAGE_SIZE")


class ResidentPeak(threading.Thread):
    def __init__(self):
        super().__init__(daemon=True)
        self.peak, self.done = resident(), False

    def run(self):
        while not self.done:
            self.peak = max(self.peak, resident())
            time.sleep(0.001)


procs = {"torch": SAMAudioProcessor.from_config(cfg), "hip": SAMAudioProcessor.from_config(cfg, audio_transform="hip", device=dev)}

with tempfile.TemporaryDirectory() as tmp:
    pcm, paths, tensors = make_clips(tmp)
    torch.zeros(1, device=dev)
    torch.cuda.synchronize()
    if memory:
        call(procs[transform], kind, paths, tensors, move=True)     # warm-up: code objects, the filter bank, the allocator's blocks
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base, rss0 = torch.cuda.memory_allocated(), resident()
        watch = ResidentPeak()
        watch.start()
        batch = call(procs[transform], kind, paths, tensors, move=True)
        watch.done = True
        watch.join()
        print(f"  memory, audio_transform={transform!r}, {kind}: resident set {rss0 / 2 ** 20:.0f} MiB before the call, peak + "
              f"{(watch.peak - rss0) / 2 ** 20:.0f} MiB during it; device peak + {(torch.cuda.max_memory_allocated() - base) / 2 ** 20:.0f} MiB, "
              f"of which the batch {batch.audios.numel() * 4 / 2 ** 20:.0f} MiB")
        sys.exit(0)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    steps = {}
    for kind in ("files", "tensors"):
        for t in ("torch", "hip"):
            steps[f"__call__, {kind}, {t}"] = lambda t=t, kind=kind: call(procs[t], kind, paths, tensors)
            steps[f"__call__ + .to(device), {kind}, {t}"] = lambda t=t, kind=kind: call(procs[t], kind, paths, tensors, move=True)
    outs = {k: clock(f)[1] for k, f in steps.items()}     # warm-up: code objects, the filter bank, the allocator's blocks
    times = {k: [] for k in steps}
    for _ in range(reps):
        for k, f in steps.items():
            times[k].append(clock(f)[0])
    print(f"{n_clips} stereo 16-bit clips of {seconds} s at {rate} Hz -> {model_rate} Hz mono, [B, 1, {outs['__call__, files, hip'].audios.shape[-1]}]; "
          f"{reps} rounds alternating in one process after a warm-up (host clock to a device synchronise, ms); "
          f"{torch.get_num_threads()} CPU threads")
    med = {k: statistics.median(v) for k, v in times.items()}
    for k in steps:
        print(f"  {k:42s} median {med[k]:9.3f}   min {min(times[k]):9.3f}   max {max(times[k]):9.3f}")
    for kind in ("files", "tensors"):
        a, b = outs[f"__call__, {kind}, torch"], outs[f"__call__, {kind}, hip"]
        err = (a.audios - b.audios.cpu()).abs().max().item()
        print(f"  {kind}: hip against torch max-abs {err:.3e}; sizes equal {torch.equal(a.sizes, b.sizes.cpu())}; "
              f"hip / torch {med[f'__call__ + .to(device), {kind}, hip'] / med[f'__call__ + .to(device), {kind}, torch']:.4f} (with .to(device))")

    # the kernel alone
    frames = [x.t().contiguous().flatten().to(dev) for x in pcm]
    length = audio.resample_length(samples, rate, model_rate)
    out = torch.empty(n_clips, 1, length, device=dev)

    def launches():
        for row, x in zip(out, frames):
            audio.mix_into(row[0], x, 2, samples, 1, 2, rate, model_rate)

    launches()
    torch.cuda.synchronize()
    ms = []
    for _ in range(max(reps, 20)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launches()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    moved = sum(x.numel() * 2 for x in frames) + out.numel() * 4
    k_med = statistics.median(ms)
    print(f"  kernel, {n_clips} launches (device events): median {k_med:.3f} ms, min {min(ms):.3f}, max {max(ms):.3f}; "
          f"{moved / 1e6:.1f} MB (int16 read + fp32 written) -> {moved / (k_med * 1e-3) / 1e12:.3f} TB/s of the 8 TB/s HBM peak")
    sys.stdout.flush()
    memory_children()
