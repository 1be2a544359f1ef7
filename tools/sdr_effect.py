#!/usr/bin/env python
"""Look at the projection SDR (buddy_amd/utils/sdr.py) on simulated rooms whose decay is known: 16 rooms from
tools/make_paired_set.py --diffuse-tail --reverberant over synthetic clean signals (``synth_clean``, 4 s).  Per room, in order of its nominal T60: the
SDR of the reverberant file against its clean signal at 1, 16, 64, 256, 512, 1024 and 2048 taps; then the rank correlation of every column with the
nominal T60.  The expectation to confirm or refute: the 2048-tap value falls with T60 while the 1-tap value barely moves.  One run, written as text
(default profiles/sdr_effect.txt).  Nothing is gated on it."""
import argparse
import importlib.util
import os
import sys
import tempfile

import numpy as np
import torch
from scipy.io import wavfile
from scipy.stats import spearmanr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from buddy_amd.synth import synth_clean  # noqa: E402
from buddy_amd.utils import sdr  # noqa: E402

TAPS = (1, 16, 64, 256, 512, 1024, 2048)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rooms", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdr_effect.txt"))
    a = ap.parse_args(argv)
    spec = importlib.util.spec_from_file_location("buddy_tools_make_paired_set", os.path.join(ROOT, "tools", "make_paired_set.py"))
    mps = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mps)
    with tempfile.TemporaryDirectory() as tmp:
        clean = os.path.join(tmp, "clean", "synth")
        os.makedirs(clean)
        for u in range(a.rooms):
            wavfile.write(os.path.join(clean, f"s{u:02d}.wav"), 16000, synth_clean(u, 64000).astype(np.float32))
        out = os.path.join(tmp, "set")
        rows = mps.main(["--clean", os.path.join(tmp, "clean"), "--out", out, "--seed", str(a.seed), "--diffuse-tail", "--reverberant", "--device", a.device])
        x, y = (np.stack([wavfile.read(os.path.join(out, sub, r["file"] + ".wav"))[1] for r in rows]) for sub in ("clean", "reverberant"))
    ev = sdr.evaluate(torch.from_numpy(y).to(a.device), torch.from_numpy(x).to(a.device), 16000, values=TAPS)
    v, t60 = ev.values.numpy(), np.array([r["eyring_T60"] for r in rows])
    lines = [f"projection SDR of the reverberant files of {a.rooms} simulated rooms against their clean signals (tools/sdr_effect.py, seed {a.seed}):",
             "make_paired_set --diffuse-tail --reverberant, synthetic clean signals of 4 s (synth_clean), taps at 16 kHz, loading 1e-9, rooms in order of their",
             "nominal (Eyring) T60; T30 and DRR as measured on the response.", "",
             f"  {'room':>10}  {'T60 s':>6}  {'T30 s':>6}  {'DRR dB':>6}  " + "  ".join(f"{'sdr' + str(m):>8}" for m in TAPS) + "  flags"]
    for b in np.argsort(t60):
        r = rows[b]
        lines.append(f"  {r['file']:>10}  {t60[b]:6.3f}  {r['T30']:6.3f}  {r['DRR']:6.2f}  " + "  ".join(f"{v[b, q]:8.3f}" for q in range(len(TAPS))) + f"  {int(ev.flags[b])}")
    lines += ["", "Spearman rank correlation with the nominal T60, and the spread over the rooms:"]
    for q, m in enumerate(TAPS):
        rho = spearmanr(t60, v[:, q])[0]
        lines.append(f"  sdr{m:<5d} rho {rho:+.3f}   min {v[:, q].min():8.3f}  median {np.median(v[:, q]):8.3f}  max {v[:, q].max():8.3f} dB")
    rise = v[:, -1] - v[:, 0]
    lines += ["", f"rise from 1 to 2048 taps: min {rise.min():.3f}  median {np.median(rise):.3f}  max {rise.max():.3f} dB; Spearman rho with T60 {spearmanr(t60, rise)[0]:+.3f}",
              "", "Speech and the output of a trained checkpoint remain unmeasured."]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
