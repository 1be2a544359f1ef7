#!/usr/bin/env python
"""Check the blind decay time (buddy_amd/utils/decay.py) on simulated rooms whose decay is known: 32 rooms from
tools/make_paired_set.py --diffuse-tail --reverberant, with and without --bands and at --snr 20 20, a gated-burst source as the "clean" signal
(speech-like gaps; the synthetic clean signal of the tests never falls silent).  Per band: the blind T60 of the reverberant file against the room's
nominal T60 and against the T30 the room-acoustics analysis measures on the response; the median and the largest relative error.  One run, written
as text (default profiles/decay_effect.txt).  Nothing is gated on it."""
import argparse
import importlib.util
import os
import sys
import tempfile

import numpy as np
from scipy.io import wavfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from buddy_amd.utils import decay  # noqa: E402


def burst_source(seed, seconds=8.0, fs=16000):
    """gated bursts of low-passed noise: on 0.12-0.4 s, off 0.15-0.5 s, 5 ms linear ramps, gains 0.3-1 (the source of the tests' functional condition)"""
    rs = np.random.RandomState(seed)
    n = int(seconds * fs)
    x = np.zeros(n)
    h = np.exp(-np.arange(64) / 8.0)
    ramp = int(0.005 * fs)
    pos = 0
    while pos < n:
        on = int(rs.uniform(0.12, 0.4) * fs)
        off = int(rs.uniform(0.15, 0.5) * fs)
        b = np.convolve(rs.standard_normal(on + 64), h)[64:64 + on]
        r = np.linspace(0.0, 1.0, ramp)
        b[:ramp] *= r
        b[-ramp:] *= r[::-1]
        b *= rs.uniform(0.3, 1.0)
        m = min(on, n - pos)
        x[pos:pos + m] = b[:m]
        pos += on + off
    return x


def rel(v, ref):
    v, ref = np.asarray(v, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    e = np.abs(v / ref - 1.0)
    e = e[~np.isnan(e)]
    return (len(e), float(np.median(e)) if len(e) else float("nan"), float(np.max(e)) if len(e) else float("nan"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rooms", type=int, default=32)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decay_effect.txt"))
    a = ap.parse_args(argv)
    spec = importlib.util.spec_from_file_location("buddy_tools_make_paired_set", os.path.join(ROOT, "tools", "make_paired_set.py"))
    mps = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mps)
    lines = [f"blind decay time of the reverberant files of {a.rooms} simulated rooms (tools/decay_effect.py, seed {a.seed}): make_paired_set --diffuse-tail",
             "--reverberant, nominal T60 0.2 .. 1.0 s, the gated-burst source (8 s) as the clean signal.  err = |t60_in / reference - 1|; n = files where the",
             "band's decay time is defined.  Without --bands the walls do not depend on frequency: every band's nominal T60 is the room's, and the",
             "response is analysed broadband only, so every band is held against the broadband T30.", ""]
    with tempfile.TemporaryDirectory() as tmp:
        clean = os.path.join(tmp, "clean", "bursts")
        os.makedirs(clean)
        for u in range(a.rooms):
            wavfile.write(os.path.join(clean, f"b{u:02d}.wav"), 16000, burst_source(u).astype(np.float32))
        for tag, extra in (("plain walls", []), ("--bands", ["--bands"]), ("plain walls, --snr 20 20", ["--snr", "20", "20"])):
            out = os.path.join(tmp, tag.replace(" ", "_").replace(",", ""))
            rows = mps.main(["--clean", os.path.join(tmp, "clean"), "--out", out, "--seed", str(a.seed), "--diffuse-tail", "--reverberant", "--device", a.device,
                             *extra])
            sigs = []
            for r in rows:
                fs, y = wavfile.read(os.path.join(out, "reverberant", r["file"] + ".wav"))
                sigs.append((y.astype(np.float32), fs))
            sc = decay.score_signals(sigs, a.device)
            lines.append(f"{tag}: {len(rows)} rooms, nominal T60 {min(r['eyring_T60'] for r in rows):.3f} .. {max(r['eyring_T60'] for r in rows):.3f} s")
            lines.append(f"  {'band':>10}  {'n':>3}  {'median t60_in':>13}  {'vs nominal: median':>18}  {'max':>6}  {'vs T30: median':>14}  {'max':>6}  {'median regions':>14}")
            for k, name in enumerate(decay.NAMES):
                f = None if k == 0 else str(decay.CENTRES[k - 1])
                banded = f is not None and ("eyring_T60_" + f) in rows[0]
                nominal = [r["eyring_T60_" + f] if banded else r["eyring_T60"] for r in rows]
                t30 = [r["T30_" + f] if banded else r["T30"] for r in rows]
                t = [s["t60"][k] for s in sc]
                n, med_n, max_n = rel(t, nominal)
                _, med_m, max_m = rel(t, t30)
                tv = np.array(t)
                lines.append(f"  {'broadband' if f is None else f + ' Hz':>10}  {n:3d}  {float(np.nanmedian(tv)) if n else float('nan'):13.3f}  {med_n:18.3f}  {max_n:6.3f}  "
                             f"{med_m:14.3f}  {max_m:6.3f}  {float(np.median([s['regions'][k] for s in sc])):14.1f}")
            lines.append("")
    lines.append("--snr with --bands is refused by make_paired_set, so the banded rooms have no noisy run.  Speech and a trained checkpoint remain unmeasured.")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
