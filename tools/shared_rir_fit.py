"""A recorded number, not a gate: does fitting ONE blind operator to the four chunks of a clip (tied rows, buddy_blindop_set_groups) recover the room
better than four operators fitted to one chunk each?  Synthetic and informed: a 4 x 1.024 s synthetic clean signal, one synthetic RIR, the whole
signal reverberated, both cut into four chunks; the operator is fitted with x_den := the CLEAN chunks (200 Adam iterations), once untied and once
as one group.  For each of the five RIR estimates: the error of its energy-decay curve against the true RIR's, in dB, and the T60 read from it.
The clean signal is given, so this says nothing about the blind chain (speech and room estimated together).
usage: python tools/shared_rir_fit.py [OUT.txt]   (default profiles/shared_rir_fit.txt)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from buddy_amd.config import compose
from buddy_amd.synth import synth_clean, synth_rir
from buddy_amd.testing.operators.subband_filtering import BlindSubbandFiltering
from buddy_amd.utils.reverb_utils import fast_apply_RIR

SR, CHUNK, N, ITERS = 16000, 16384, 4, 200


def edc_db(h):
    """Schroeder energy-decay curve, 0 dB at t = 0"""
    e = np.cumsum((np.asarray(h, np.float64) ** 2)[::-1])[::-1]
    return 10.0 * np.log10(e / e[0] + 1e-30)


def t60_of(edc):
    """T20 x 3: line through the -5 .. -25 dB stretch of the decay curve"""
    i = np.nonzero((edc <= -5.0) & (edc >= -25.0))[0]
    if len(i) < 2:
        return float("nan")
    slope = np.polyfit(i / SR, edc[i], 1)[0]
    return -60.0 / slope


def main(out_path):
    args = compose(tester="blind_dereverberation_BUDDy")
    ps = args.tester.posterior_sampling
    per_call = int(ps.blind_hp.op_updates_per_step)
    x = torch.from_numpy(synth_clean(0, N * CHUNK)).cuda()
    h = synth_rir(0, 8000)
    y = fast_apply_RIR(x[None], torch.from_numpy(h).cuda())[0]
    xs, ys = x.reshape(N, CHUNK).contiguous(), y.reshape(N, CHUNK).contiguous()
    true = edc_db(h)
    span = np.nonzero(true >= -40.0)[0][-1] + 1        # compare the curves down to -40 dB of the true one
    lines = [f"true RIR: T60 {t60_of(true):.3f} s; decay curves compared over the first {span / SR:.3f} s (true curve down to -40 dB); "
             f"{ITERS} Adam iterations, x_den = the clean chunks"]
    for label, groups in (("untied", None), ("tied", [0] * N)):
        torch.manual_seed(0)
        op = BlindSubbandFiltering(args.tester.informed_dereverberation.op_hp, sample_rate=SR, num_utts=N, device="cuda", length=CHUNK, groups=groups)
        op.update_H(use_noise=True)
        op.hip_bind(ys, ps)
        for _ in range(ITERS // per_call):
            op.hip_optimize(xs, float(ps.RIR_noise_regularization.crop_sigma_min))
        op.update_H()
        rirs = op.get_time_RIR().detach().cpu().numpy()
        for u in range(1 if groups else N):
            e = edc_db(rirs[u])
            err = np.abs(e[:span] - true[:span])
            lines.append(f"{label} {'group of ' + str(N) if groups else 'chunk ' + str(u)}: decay-curve error mean {err.mean():.2f} dB, max {err.max():.2f} dB; "
                         f"T60 {t60_of(e):.3f} s")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "shared_rir_fit.txt"))
