"""Timing of the CLAP ranker on one GPU (profiles/clap/README.md): `python tools/clap_probe.py [clips candidates seconds rounds]`.

HTSAT-tiny / RoBERTa-base dims with seeded random weights (sam_audio_amd/synthetic.py init_clap_model: the arithmetic does not depend
on the values), `clips` x `candidates` waveforms of `seconds` at 48 kHz, one prompt per clip:
  forward   ClapRanker.forward between device events, median / min / max over `rounds` after a warm-up
  parts     the same for the front end alone, audio_embed and text_embed
`python tools/clap_probe.py kernels`: one warm-up and one forward of 8 x 8 x 10 s, for a kernel trace (rocprofv3 --kernel-trace --stats).
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from sam_audio_amd import clap, synthetic  # noqa: E402
from sam_audio_amd.ranking import ClapRanker  # noqa: E402


class Tokenizer:
    def __call__(self, texts, padding=True, truncation=True, max_length=None, return_tensors="pt"):
        rows = [[0] + [3 + ord(c) % 5000 for c in t][: (max_length or 512) - 2] + [2] for t in texts]
        T = max(map(len, rows))
        ids = torch.tensor([r + [1] * (T - len(r)) for r in rows])
        return {"input_ids": ids, "attention_mask": (ids != 1).long()}


def timed(fn, rounds):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    trace = len(sys.argv) > 1 and sys.argv[1] == "kernels"
    clips, cands, seconds, rounds = (8, 8, 10, 1) if trace else [int(v) for v in (sys.argv[1:5] + ["8", "8", "10", "10"][len(sys.argv) - 1:])]
    dev = torch.device("cuda:0")
    tower = clap.ClapTower.from_module(synthetic.init_clap_model(synthetic.clap_config("real"), seed=0), dev)
    ranker = ClapRanker(model=tower, tokenizer=Tokenizer())
    n = seconds * 48_000
    wavs = [torch.stack([synthetic.synthetic_clip(8 * b + c, n)[0] for c in range(cands)]).to(dev) for b in range(clips)]
    prompts = [f"the sound of thing number {b} in a room" for b in range(clips)]
    scores = ranker(extracted_audio=wavs, descriptions=prompts, sample_rate=48_000)
    torch.cuda.synchronize()
    print(f"{clips} clips x {cands} candidates x {seconds} s at 48 kHz, HTSAT-tiny / RoBERTa-base dims; scores {tuple(scores.shape)}, "
          f"finite {bool(torch.isfinite(scores).all())}")
    if trace:
        ranker(extracted_audio=wavs, descriptions=prompts, sample_rate=48_000)
        torch.cuda.synchronize()
        return
    flat = torch.cat(wavs)
    tok = Tokenizer()(prompts)
    ids, mask = tok["input_ids"].to(dev), tok["attention_mask"].to(dev)
    for name, fn in (("ClapRanker.forward", lambda: ranker(extracted_audio=wavs, descriptions=prompts, sample_rate=48_000)),
                     (f"front end alone ({clips * cands} rows, one call)", lambda: tower.logmel(flat)),
                     (f"audio_embed ({clips} calls of {cands} rows)", lambda: [tower.audio_embed(w) for w in wavs]),
                     (f"text_embed ({clips} rows x {ids.shape[1]} tokens)", lambda: tower.text_embed(ids, mask))):
        med, lo, hi = timed(fn, rounds)
        print(f"  {name}: median {med:.2f} ms, min {lo:.2f}, max {hi:.2f} over {rounds} rounds (device events)")


if __name__ == "__main__":
    main()
