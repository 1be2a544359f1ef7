"""GPU: tools/make_paired_set.py with the noise flags, end to end on two synthetic files of one second and a 4-microphone
array: reproducible bytes, ``reverberant - noise`` = the noiseless run, the SNR that was asked for, and a run without the flags that writes what it
wrote before the flags existed."""
import csv
import filecmp
import math
import os
import sys

import numpy as np
import pytest
from scipy.io import wavfile

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("p1/a", "p1/b")
COMMON = ["--mics", "4", "--reverberant", "--rir-seconds", "0.2", "--max-order", "3", "--seed", "3"]
NOISE = ["--snr", "10", "20", "--sensor-snr", "30", "--noise-waves", "32"]
NEW_COLUMNS = ("snr_db", "snr_reference", "snr_measured_db", "noise_gain_diffuse", "noise_gain_sensor", "noise_flags")


def files_under(base):
    return sorted(os.path.relpath(os.path.join(d, f), base) for d, _, fs in os.walk(base) for f in fs)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{"noisy", "again", "plain"} -> folder: the same call twice, and the call without the noise flags"""
    from buddy_amd.synth import synth_clean
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_paired_set as T
    base = tmp_path_factory.mktemp("noise_set")
    os.makedirs(base / "clean_in" / "p1")
    for u, name in enumerate(NAMES):
        wavfile.write(str(base / "clean_in" / (name + ".wav")), 16000, synth_clean(u, 16000))
    out = {}
    for tag, extra in (("noisy", NOISE), ("again", NOISE), ("plain", [])):
        out[tag] = str(base / tag)
        T.main(["--clean", str(base / "clean_in"), "--out", out[tag]] + COMMON + extra)
    return out


def wav(base, sub, name):
    fs, a = wavfile.read(os.path.join(base, sub, name + ".wav"))
    assert fs == 16000 and a.dtype == np.float32
    return a


def test_two_runs_are_byte_identical(runs):
    names = files_under(runs["noisy"])
    assert names == files_under(runs["again"]) and sum(n.startswith("noise" + os.sep) for n in names) == 2
    for n in names:
        assert filecmp.cmp(os.path.join(runs["noisy"], n), os.path.join(runs["again"], n), shallow=False), n


def test_without_the_flags_nothing_changes(runs):
    plain = files_under(runs["plain"])
    assert not os.path.exists(os.path.join(runs["plain"], "noise")) and len(plain) == len(files_under(runs["noisy"])) - 2
    header = open(os.path.join(runs["plain"], "rooms.csv")).readline().strip().split(",")
    assert not set(NEW_COLUMNS) & set(header) and header[-3:] == ["mics", "array_radius", "array_angle"]
    noisy_header = open(os.path.join(runs["noisy"], "rooms.csv")).readline().strip().split(",")
    assert noisy_header == header + list(NEW_COLUMNS)
    for n in plain:                                  # the noise touches reverberant/ and rooms.csv only
        if not n.startswith("reverberant") and n != "rooms.csv":
            assert filecmp.cmp(os.path.join(runs["plain"], n), os.path.join(runs["noisy"], n), shallow=False), n


def test_reverberant_minus_noise_is_the_noiseless_file(runs):
    for name in NAMES:
        mixed, nz, y = wav(runs["noisy"], "reverberant", name), wav(runs["noisy"], "noise", name), wav(runs["plain"], "reverberant", name)
        assert mixed.shape == nz.shape == y.shape == (len(y), 4) and np.abs(nz).max() > 0
        diff = np.abs(mixed.astype(np.float64) - nz.astype(np.float64) - y.astype(np.float64))
        assert np.all(diff <= 2.0 ** -24 * np.abs(mixed))            # mixed = fp32(y + noise): one rounding
        r = np.corrcoef(nz.T)                                                # not four copies of one signal
        assert abs(r[0, 1]) < 0.99 and not np.array_equal(nz[:, 0], nz[:, 1])


def test_the_snr_is_the_one_asked_for(runs):
    with open(os.path.join(runs["noisy"], "rooms.csv"), newline="") as f:
        rows = {r["file"]: r for r in csv.DictReader(f)}
    assert sorted(rows) == sorted(NAMES)
    for name in NAMES:
        r = rows[name]
        asked = float(r["snr_db"])
        assert 10.0 <= asked <= 20.0 and r["snr_reference"] == "rms" and abs(float(r["snr_measured_db"]) - asked) < 1e-3
        assert float(r["noise_gain_diffuse"]) > 0 and float(r["noise_gain_sensor"]) > 0 and r["noise_flags"] == ""
        mixed, nz = wav(runs["noisy"], "reverberant", name).astype(np.float64), wav(runs["noisy"], "noise", name).astype(np.float64)
        snr = 10.0 * math.log10(np.sum((mixed[:, 0] - nz[:, 0]) ** 2) / np.sum(nz[:, 0] ** 2))
        print(f"{name}: snr_db {asked:.6f}, recomputed from the files {snr:.6f}")
        assert abs(snr - asked) < 1e-3
    assert rows[NAMES[0]]["snr_db"] != rows[NAMES[1]]["snr_db"]
