"""Per-launch times of the gemm = "f16" kernels against their f16x2-mode counterparts, from a rocprofv3 kernel trace of tools/gemm_f16_leg.py (both legs in
one process; same layers in the same order).
usage: rocprofv3 --kernel-trace --output-format csv -d DIR -o f16 -- python tools/gemm_f16_leg.py --rounds 1 --steps 3 --warmup 1
       python tools/gemm_f16_trace.py DIR/.../f16_kernel_trace.csv
The f16 input transform has no channel-block grid axis (a workgroup walks all channels of its tiles), so its launches cannot be told apart by grid; they
are paired in launch order with the fp32 input-transform launches of the f16x2 leg of the same form and tile count (the same convolutions: the f16x2
leg's extra first forward comes first and is skipped), whose grid y gives K = 128 x blocks.  GEMMs pair by grid (same formula in both kernels)."""
import collections
import csv
import re
import statistics
import sys


def form(name):
    """(kind, GN, S2D, TS) of an input transform (demangled or mangled name), ('gemm16' | 'gemm16x2',) of a batched GEMM, else None"""
    if "w6_input_f16_kernel" in name:
        m = re.search(r"w6_input_f16_kernel(?:<(\d), (true|false), (\d)>|ILi(\d)ELb(\d)ELi(\d)E)", name)
        g = m.groups()
        return ("in16", int(g[0]), g[1] == "true", int(g[2])) if g[0] else ("in16", int(g[3]), g[4] == "1", int(g[5]))
    m = re.search(r"w6_input_kernel<(\d), (true|false), (\d)>", name)
    if m:
        return ("in32", int(m.group(1)), m.group(2) == "true", int(m.group(3)))
    if "wgemm_f16_kernel" in name:
        return ("gemm16",)
    if "wgemm_f16x2_rt2_kernel" in name:
        return ("gemm16x2",)
    return None


def main(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    seq = collections.defaultdict(list)            # (kind, form..., tiles) -> [(grid y, us)]
    for r in rows:
        f = form(r["Kernel_Name"])
        if f is None:
            continue
        gx = int(r.get("Grid_Size_X", r.get("Grid_Size", 0))) // int(r.get("Workgroup_Size_X", r.get("Workgroup_Size", 256)))
        gy = int(r.get("Grid_Size_Y", 1))
        us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
        seq[f[:1] + f[1:] + (gx,)].append((gy, us))
    print(f"{'kernel':44s} {'grid x':>7s} {'K':>5s} {'n':>4s} {'f16x2 mode us':>14s} {'f16 us':>8s} {'ratio':>6s}")
    for key, l16 in sorted(seq.items()):
        if key[0] == "in16":
            l32 = seq.get(("in32",) + key[1:], [])[-len(l16):]
            if len(l32) != len(l16):
                print("unpaired", key, len(l16), len(l32)); continue
            by = collections.defaultdict(lambda: ([], []))
            for (gy, us32), (_, us16) in zip(l32, l16):
                by[gy][0].append(us32); by[gy][1].append(us16)
            for gy, (a, b) in sorted(by.items()):
                name = f"w6_input{{,_f16}}_kernel<{key[1]}, {str(key[2]).lower()}, {key[3]}>"
                print(f"{name:44s} {key[4]:7d} {128 * gy:5d} {len(b):4d} {statistics.median(a):14.1f} {statistics.median(b):8.1f} {statistics.median(b) / statistics.median(a):6.2f}")
        elif key[0] == "gemm16":
            a = [us for _, us in seq.get(("gemm16x2", key[1]), [])]
            b = [us for _, us in l16]
            if a:
                print(f"{'wgemm_f16x2_rt2_kernel / wgemm_f16_kernel':44s} {key[1]:7d} {'':>5s} {len(b):4d} {statistics.median(a):14.1f} {statistics.median(b):8.1f} "
                      f"{statistics.median(b) / statistics.median(a):6.2f}")


if __name__ == "__main__":
    main(sys.argv[1])
