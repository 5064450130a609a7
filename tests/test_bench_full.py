"""bench.py --full: a plain run does only what the headline figure needs (set up, warm up, time the steps, --dump-outputs, the JSON
line); everything else the benchmark measures or checks - rooflines, cpu_baseline, parity_check, hostile_check, the plain 16-bit
modes side by side, other_configs, the other scaling mode, rerank_breakdown, vision_tower - runs with --full only, where the --no-*
switches still trim it."""
import json
import os
import subprocess
import sys
import time

import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_switches_every_extra_off():
    args = bench.parse(["--gpus", "1", "--steps", "4", "--warmup", "2"])
    assert not args.full and (args.steps, args.warmup) == (4, 2)
    assert all(getattr(args, extra) for extra in bench.EXTRAS)
    # the workload of the timed steps is the same with and without --full
    full = bench.parse(["--gpus", "1", "--steps", "4", "--warmup", "2", "--full"])
    differ = {k for k in vars(args) if getattr(args, k) != getattr(full, k)}
    assert differ == {"full", *bench.EXTRAS}
    assert bench.default_workload(args) and bench.default_workload(full)


def test_full_run_keeps_every_extra_and_its_switch():
    args = bench.parse(["--full"])
    assert args.full and not any(getattr(args, extra) for extra in bench.EXTRAS)
    args = bench.parse(["--full", "--no-cpu-baseline", "--verify", "--no-other-configs"])
    assert args.no_cpu_baseline and args.verify and args.no_other_configs
    assert not (args.no_roofline or args.no_verify or args.no_parity_mode or args.no_hostile or args.no_other)


def test_extras_cover_every_no_switch():
    """a --no-* switch added later without a line in EXTRAS would leave its section running in a plain run"""
    args = vars(bench.parse(["--full"]))
    assert {k for k in args if k.startswith("no_")} == set(bench.EXTRAS)


def test_verify_needs_full():
    with pytest.raises(SystemExit):
        bench.parse(["--no-cpu-baseline", "--verify"])


def test_other_configs_sub_runs_ask_for_full(monkeypatch):
    """the sub-lines carry their own roofline and parity_check, so the sub-processes are --full runs"""
    seen = []

    def fake_run(cmd, **kw):
        seen.append(cmd)
        sub = bench.parse(cmd[2:])
        assert sub.full and sub.verify and sub.no_other_configs and sub.no_cpu_baseline and not sub.no_roofline
        return subprocess.CompletedProcess(cmd, 0, stdout=json.dumps({"value": 1.0, "unit": "s-audio/s"}) + "\n", stderr="")

    monkeypatch.setattr(subprocess, "run", fake_run)
    out = bench.other_configs(bench.parse(["--full"]))
    assert len(seen) == len(out) == 4 and all("error" not in o for o in out)


@pytest.mark.gpu
def test_plain_run_on_the_gpu_prints_the_headline_only(gpu, tmp_path):
    """small* dims, 2 clips: the line keeps its headline keys, the sections of --full are null, and the run spends little outside
    its steps (the 30 s bound of a plain run, on the whole process from start to exit)."""
    if gpu.type != "cuda":
        pytest.skip("bench.py runs in a process of its own, on a real GPU")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--size", "small*", "--batch", "2",
           "--dump-outputs", str(tmp_path)]
    t0 = time.perf_counter()
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stderr[-2000:]
    rows = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(rows) == 1
    line = json.loads(rows[0])
    assert line["metric"] == "seconds-of-audio separated/sec/node" and line["unit"] == "s-audio/s" and line["higher_is_better"] is True
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["dtype"].startswith("fp16x3")
    assert (line["steps"], line["warmup"], line["full"]) == (2, 1, False)
    for key in ("roofline", "roofline_hbm", "kernels", "cpu_baseline", "parity_check", "hostile_check", "other_scaling", "rerank_breakdown",
                "vision_tower", "fp16_mode", "bf16_mode"):
        assert line[key] is None, key
    assert "other_configs" not in line
    assert sorted(os.listdir(tmp_path)) == ["noise.npy", "residual.npy", "target.npy"]
    outside = wall - 3 * line["ms_per_step"] / 1e3
    print(f"plain run: wall {wall:.1f} s, {outside:.1f} s outside its 3 steps")
    assert outside <= 30.0
