"""GPU: the active speech level (csrc/level.hip behind the C entries, buddy_amd/utils/level.py) against the float64 restatement
of tests/_level_ref.py.  A comparison against a threshold is a decision, so the GPU's counts must EQUAL the restatement's; tests/test_level_host.py
asserts that on every seed used here the restatement's counts do not move when every threshold moves by +-eps, the derived bound on the two
envelopes' difference, so no case needs the "in between" branch.  sq, level_db and activity are held to the tolerances derived in _level_ref.py.
Then: the hangover edge on hand-made class bytes, activity known from construction, the step response's closed form, gains, the two full scales,
every flag between valid neighbours, batch = solo, run = run, every refused argument, and the real-recordings mode with ``level: active``."""
import math
import os
import sys

import numpy as np
import pytest
import torch
from scipy.io import wavfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _level_ref as R  # noqa: E402
from buddy_amd import _lib  # noqa: E402
from buddy_amd.utils import level as lv  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY, SENTINEL = 0xA5, -7.0
U = 2.0 ** -53
_REF = {}
WORST = {"sq": 0.0, "level_db": 0.0, "activity": 0.0}      # largest observed error / bound, printed by the tests that update them


@pytest.fixture(scope="module")
def lib():
    return _lib.require_gpu()


def tiles(lib):
    return int(lib.buddy_level_tile()), int(lib.buddy_level_counts_tile())


def ref_of(lib, name):
    """the restatement of every row of a seeded case, computed once"""
    if name not in _REF:
        T, Tc = tiles(lib)
        fs, rows, remove_mean = R.gpu_cases(T, Tc)[name]
        _REF[name] = (fs, rows, remove_mean, [R.level_ref(x, fs, remove_mean=remove_mean, T=T) for x in rows])
    return _REF[name]


def _ws(query, B, longest):
    nbytes = int(query(B, longest))
    assert nbytes >= 0
    return torch.zeros(max(nbytes // 8, 1), dtype=torch.float64, device="cuda"), nbytes


def padded(rows, ldx, garbage=float("nan")):
    """(B, ldx) float32 on the GPU with garbage behind every row's end, and the lengths"""
    x = np.full((len(rows), ldx), garbage, dtype=np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return torch.from_numpy(x).cuda(), [len(r) for r in rows]


def abi_classes(lib, x, lens, offset, ref, fs, ldk, tc=0.03):
    B, ldx = x.shape
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    off_d = None if offset is None else torch.tensor(offset, dtype=torch.float64, device="cuda")
    ref_d = torch.tensor(ref, dtype=torch.float64, device="cuda")
    klass = torch.full((B, ldk), CANARY, dtype=torch.uint8, device="cuda")
    sq = torch.full((B,), SENTINEL, dtype=torch.float64, device="cuda")
    ws, nbytes = _ws(lib.buddy_level_classes_workspace, B, max(lens))
    rc = lib.buddy_level_classes(x.data_ptr(), ldx, lens_d.data_ptr(), None if off_d is None else off_d.data_ptr(), ref_d.data_ptr(), B, float(fs), tc,
                                 klass.data_ptr(), ldk, sq.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, klass, sq.cpu().numpy()


def abi_counts(lib, klass, lens, hang):
    B, ldk = klass.shape
    lens_d = torch.tensor(lens, dtype=torch.int32, device="cuda")
    counts = torch.full((B, 16), -1, dtype=torch.int64, device="cuda")
    ws, nbytes = _ws(lib.buddy_level_counts_workspace, B, max(lens))
    rc = lib.buddy_level_counts(klass.data_ptr(), ldk, lens_d.data_ptr(), B, int(hang), counts.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, counts.cpu().numpy()


def classes_of(q, thresholds):
    return np.sum(np.asarray(q)[:, None] >= np.asarray(thresholds)[None, :], axis=1)


@pytest.mark.parametrize("name", ["lengths_1k", "long_8k", "hang_over_tile_48k", "batch_2k"])
@pytest.mark.parametrize("aligned", [False, True])
def test_counts_equal_the_restatement(lib, name, aligned):
    """ragged rows in one batch (n in {1, 2, I, I + 1, T - 1, T, T + 1, 2T + 3}; 40 tiles; I above the tile at 48 kHz), NaN behind every row's end and
    canary bytes behind every row of classes, strides that take the scalar and the 16-byte paths"""
    T, Tc = tiles(lib)
    fs, rows, remove_mean, refs = ref_of(lib, name)
    longest = max(len(r) for r in rows)
    ldx = (longest + 15) // 16 * 16 + 16 if aligned else longest + 3
    ldk = ldx if aligned else longest + 5
    x, lens = padded(rows, ldx)
    rc, klass, sq = abi_classes(lib, x, lens, [r["o"] for r in refs] if remove_mean else None, [r["R"] for r in refs], fs, ldk)
    assert rc == 0, lib.buddy_last_error()
    kl = klass.cpu().numpy()
    rc, counts = abi_counts(lib, klass, lens, refs[0]["hang"])
    assert rc == 0, lib.buddy_last_error()
    for b, r in enumerate(refs):
        n = r["n"]
        assert (kl[b, n:] == CANARY).all(), f"row {b}: a class byte was written behind the row's end"
        assert r["counts_up"] == r["counts"] == r["counts_down"]
        assert counts[b].tolist() == r["counts"], (name, b, n)
        want = classes_of(r["q"], r["thresholds"])
        near = (np.abs(r["q"][:, None] - np.asarray(r["thresholds"])[None, :]) <= r["eps"]).any(axis=1)
        assert (kl[b, :n][~near] == want[~near]).all() and near.sum() <= 2
        rel = abs(sq[b] - r["sq"]) / r["sq"]
        WORST["sq"] = max(WORST["sq"], rel / R.tol_sq_rel(n, T))
        assert rel <= R.tol_sq_rel(n, T), (name, b, rel)
    print(f"{name} aligned={aligned}: sq error / bound so far {WORST['sq']:.3f}")
    # the whole meter: the offset and the peak now come from the GPU's own row statistics
    res = lv.speech_level(x, fs, lengths=lens, remove_mean=remove_mean)
    for b, r in enumerate(refs):
        assert res.counts[b].tolist() == r["counts"] and int(res.flags[b]) == r["flags"], (name, b)
        assert float(res.peak[b]) == pytest.approx(r["R"], rel=64 * U)
        if math.isnan(r["level_db"]):
            assert math.isnan(float(res.level_db[b]))
            continue
        e_l, e_a = abs(float(res.level_db[b]) - r["level_db"]), abs(float(res.activity[b]) - r["activity"])
        WORST["level_db"] = max(WORST["level_db"], e_l / R.tol_level(r, T))
        WORST["activity"] = max(WORST["activity"], e_a / R.tol_activity(r, T))
        assert e_l <= R.tol_level(r, T) and e_a <= R.tol_activity(r, T), (name, b, e_l, e_a)
        assert float(res.rms_db[b]) == pytest.approx(r["rms_db"], abs=R.tol_level(r, T))
        assert float(res.active_rms[b]) == pytest.approx(10.0 ** (r["level_db"] / 20.0), rel=1e-12)
    print(f"{name} aligned={aligned}: level_db error / bound so far {WORST['level_db']:.3f}, activity {WORST['activity']:.3f}")


def _window_counts(k, hang):
    return R.counts_of(np.asarray(k, dtype=np.float64), [j + 0.5 for j in range(16)], hang)


@pytest.mark.parametrize("hang", [0, 200, 9600, 2 ** 31 - 1])
def test_hangover_edge_on_hand_made_classes(lib, hang):
    """class bytes given directly: a burst whose last sample lies exactly I and I + 1 samples before a tile boundary and I - 1, I, I + 1 samples before
    the row's end, one sample of every class, random sparse classes; I = 0, below a tile, above two tiles, and beyond any row.  Integer, so equal."""
    T, Tc = tiles(lib)
    I = min(hang, 3 * Tc)
    edge = 3 * Tc if I >= Tc else 2 * Tc
    rows = []
    for d in (I, I + 1):
        k = np.zeros(edge + 40, dtype=np.uint8)
        k[max(edge - d - 30, 0):edge - d] = 16           # its last sample is d samples in front of sample `edge`, the first of a tile
        k[5] = 7
        rows.append(k)
    for d in (I - 1, I, I + 1):
        e = Tc + 11
        k = np.zeros(e + 1 + max(d, 0), dtype=np.uint8)  # the row ends max(d, 0) samples behind the burst's last sample
        k[e - 20:e + 1] = 9
        rows.append(k)
    k = np.zeros(2 * Tc + 3, dtype=np.uint8)
    k[np.arange(17) * 150 + 3] = np.arange(17)[::-1]      # one sample of every class, descending
    rows.append(k)
    rs = np.random.RandomState(hang % 1000)
    k = rs.randint(0, 17, size=3 * Tc + 1).astype(np.uint8) * (rs.uniform(size=3 * Tc + 1) < 0.002)
    rows += [k.astype(np.uint8), np.full(1, 16, dtype=np.uint8), np.zeros(Tc, dtype=np.uint8)]
    lens = [len(r) for r in rows]
    ldk = max(lens) + 7
    kl = np.full((len(rows), ldk), 16, dtype=np.uint8)     # behind the rows: the highest class, which would count if it were read
    for b, r in enumerate(rows):
        kl[b, :len(r)] = r
    rc, counts = abi_counts(lib, torch.from_numpy(kl).cuda(), lens, hang)
    assert rc == 0, lib.buddy_last_error()
    for b, r in enumerate(rows):
        assert counts[b].tolist() == _window_counts(r, min(hang, len(r))), (hang, b, len(r))


def test_activity_of_bursts_known_from_construction(lib):
    """three sine bursts of 1 s with 1 s pauses at 8 kHz: the active samples are the bursts, each followed by the hangover I and the envelope's fall to the
    deciding threshold, which lies 15.9 dB below the level, i.e. at about 0.16 of the burst's mean |x|: the two-pole fall takes less than
    5 tc (e^-5 (1 + 5) = 0.04), and its rise to it at a burst's start less than tc (1 - e^-1 (1 + 1) = 0.26).  So
    bursts (on + I - tc fs) <= a <= bursts (on + I + 5 tc fs), and the level lies below the bursts' rms by 10 log10(a / (bursts on))."""
    fs, on, bursts = 8000, 8000, 3
    I, fall = 1600, int(5 * 0.03 * fs)
    n = 2 * on * bursts
    x = np.zeros(n, dtype=np.float32)
    t = np.arange(on)
    for k in range(bursts):
        x[2 * k * on:(2 * k + 1) * on] = 0.5 * np.sin(2 * np.pi * 440.0 * t / fs)
    res = lv.speech_level(torch.from_numpy(x).cuda(), fs, remove_mean=False)
    assert int(res.flags[0]) == 0
    burst_rms_db = 10 * math.log10(float(np.sum(x.astype(np.float64) ** 2)) / (bursts * on))
    lo, hi = bursts * (on + I - int(0.03 * fs)) / n, bursts * (on + I + fall) / n
    act, level = float(res.activity[0]), float(res.level_db[0])
    print(f"activity {act:.5f} in [{lo:.5f}, {hi:.5f}]; level {level:.4f} dB, bursts' rms {burst_rms_db:.4f} dB")
    assert lo - 1e-12 <= act <= hi
    assert burst_rms_db - 10 * math.log10(hi * n / (bursts * on)) <= level <= burst_rms_db - 10 * math.log10(lo * n / (bursts * on)) + 1e-9


def test_constant_signal_follows_the_closed_form(lib):
    """x = c: p_i = c (1 - g^(i + 1)), q_i = c (1 - g^(i + 1) (1 + (i + 1) (1 - g))), the two-pole step response; the class bytes are those of the closed
    form wherever it keeps eps (plus its own few roundings) away from every threshold"""
    T, Tc = tiles(lib)
    fs, tc, c, n = 1000, 0.03, 0.3, T + 77
    x = torch.full((1, n + 1), c, dtype=torch.float32, device="cuda")
    rc, klass, sq = abi_classes(lib, x, [n], None, [1.0], fs, n + 9)
    assert rc == 0, lib.buddy_last_error()
    c = float(np.float32(c))
    g = math.exp(-1.0 / (fs * tc))
    i1 = np.arange(1, n + 1, dtype=np.float64)
    q = c * (1.0 - g ** i1 * (1.0 + i1 * (1.0 - g)))
    thr = np.array([2.0 ** (j - 15) for j in range(16)])
    eps = R.eps_kernel(fs, tc, 1.0, T) + 2.0 * (tc * fs + 1.0) * U + 8 * U      # the closed form itself: g's 2 u through |dq / dg|, and its own operations
    near = (np.abs(q[:, None] - thr[None, :]) <= eps).any(axis=1)
    got = klass.cpu().numpy()[0]
    assert (got[:n][~near] == classes_of(q, thr)[~near]).all() and near.sum() <= 1
    assert got[0] == classes_of(q[:1], thr)[0] and got[n - 1] == 14 and (got[n:] == CANARY).all()      # 0.3 lies between 2^-2 and 2^-1
    assert sq[0] == pytest.approx(n * c * c, rel=R.tol_sq_rel(n, T))


def test_gain_moves_the_level_by_20_log10(lib):
    """gains 0.5 and 2 scale every sample, the sum, the peak and every threshold exactly: the counts are equal, sq scales by exactly the square, and
    level_db moves by 20 log10(gain) up to the roundings of the finish (32 of values at most `scale`, passed on by the interpolation)"""
    T, Tc = tiles(lib)
    fs, rows, _, refs = ref_of(lib, "batch_2k")
    x = torch.from_numpy(rows[0]).cuda()
    base = lv.speech_level(x, fs)
    tol = (1.0 + refs[0]["cond"]) * 64 * U * (refs[0]["scale"] + 7.0)
    for gain in (0.5, 2.0):
        res = lv.speech_level(x * gain, fs)
        assert res.counts.tolist() == base.counts.tolist() and int(res.flags[0]) == 0
        assert float(res.peak[0]) == gain * float(base.peak[0])
        d = float(res.level_db[0]) - float(base.level_db[0])
        print(f"gain {gain}: level moved by {d!r}, 20 log10 = {20 * math.log10(gain)!r}")
        assert abs(d - 20 * math.log10(gain)) <= tol
        assert abs(float(res.activity[0]) - float(base.activity[0])) <= float(base.activity[0]) * tol


def test_full_scale_one_against_peak(lib):
    """a row whose peak is exactly 0.5, no mean removed: the peak rule's grid is the fixed grid of full scale 1 moved by one threshold, so
    counts_peak[j] == counts_one[j - 1], and the level, interpolated between the same two thresholds, is the same"""
    fs, x = R.half_peak_row(*tiles(lib))
    xg = torch.from_numpy(x).cuda()
    peak, one = lv.speech_level(xg, fs, remove_mean=False), lv.speech_level(xg, fs, full_scale=1.0, remove_mean=False)
    assert float(peak.peak[0]) == 0.5 and float(one.peak[0]) == 1.0
    assert peak.counts[0, 1:].tolist() == one.counts[0, :15].tolist()
    assert int(peak.flags[0]) == 0 and int(one.flags[0]) == 0
    assert float(peak.level_db[0]) == pytest.approx(float(one.level_db[0]), abs=1e-9)
    ref = R.level_ref(x, fs, R=1.0, remove_mean=False, T=tiles(lib)[0])
    assert ref["counts_up"] == ref["counts"] == ref["counts_down"] == one.counts[0].tolist()


def _flag_rows(fs):
    """(row, full scale or None for the peak rule, expected flags)"""
    rs = np.random.RandomState(5)
    noise = rs.standard_normal(6000).astype(np.float32) * 0.1
    clicks = np.zeros(6000, dtype=np.float32)
    clicks[::400] = 1.0                                 # crest factor 26 dB: the level is far above a threshold the envelope never reaches
    bad = noise.copy()
    bad[1234] = np.nan
    return [(R.speechlike(31, 5000, fs), None, 0), (noise, 1300.0, R.BELOW), (R.speechlike(32, 9000, fs), None, 0), (noise, 1e6, R.BELOW | R.UNDEFINED),
            (noise, 1e-3, R.ABOVE), (clicks, None, R.EDGE), (np.zeros(3000, dtype=np.float32), None, R.UNDEFINED), (bad, None, R.UNDEFINED),
            (np.zeros(0, dtype=np.float32), None, R.UNDEFINED), (R.speechlike(33, 4097, fs), None, 0)]


def test_every_flag_between_valid_neighbours(lib):
    """BELOW, BELOW with nothing active, ABOVE, EDGE, all-zero, a NaN sample and n = 0 in one batch with valid rows, which stay bit-equal to their
    solo runs"""
    fs, T = 2000, tiles(lib)[0]
    spec = _flag_rows(fs)
    scales = []
    for x, full, want in spec:                          # one number per row: the peak rule's own value where the row asks for it
        xs = x.astype(np.float64)
        scales.append(full if full is not None else (float(np.nanmax(np.abs(xs))) + abs(float(np.nanmean(xs))) if len(x) and np.nanmax(np.abs(xs)) > 0 else 1.0))
    x, lens = padded([s[0] for s in spec], max(len(s[0]) for s in spec) + 5, garbage=3.0e38)
    res = lv.speech_level(x, fs, lengths=lens, full_scale=torch.tensor(scales, dtype=torch.float64))
    for b, (row, full, want) in enumerate(spec):
        if len(row) and np.all(np.isfinite(row)):
            assert R.level_ref(row, fs, R=scales[b], T=T)["flags"] == want, f"row {b}: the restatement flags it differently"
        assert int(res.flags[b]) == want, (b, lv.flag_text(res.flags[b]))
        assert math.isnan(float(res.level_db[b])) == bool(want & R.UNDEFINED)
        if want == 0:
            solo = lv.speech_level(torch.from_numpy(row).cuda(), fs, full_scale=scales[b])
            for name in ("level_db", "activity", "active_rms", "rms_db", "counts"):
                assert torch.equal(getattr(res, name)[b], getattr(solo, name)[0]), (b, name)


def test_batch_equals_solo_and_run_equals_run(lib):
    fs, rows, _, refs = ref_of(lib, "batch_2k")
    ldx = max(len(r) for r in rows) + 1
    x, lens = padded(rows, ldx)
    offset, ref = [r["o"] for r in refs], [r["R"] for r in refs]
    rc, k1, sq1 = abi_classes(lib, x, lens, offset, ref, fs, ldx)
    rc2, k2, sq2 = abi_classes(lib, x, lens, offset, ref, fs, ldx)
    assert rc == 0 and rc2 == 0 and torch.equal(k1, k2) and (sq1 == sq2).all()
    _, c1 = abi_counts(lib, k1, lens, refs[0]["hang"])
    for b, r in enumerate(rows):
        xs, _ = padded([r], len(r) + 16)
        rc, ks, sqs = abi_classes(lib, xs, [len(r)], [offset[b]], [ref[b]], fs, len(r) + 16)
        assert rc == 0 and torch.equal(ks[0, :len(r)], k1[b, :len(r)]) and sqs[0] == sq1[b]
        _, cs = abi_counts(lib, ks, [len(r)], refs[0]["hang"])
        assert cs[0].tolist() == c1[b].tolist()
    a, b2 = lv.speech_level(x, fs, lengths=lens), lv.speech_level(x, fs, lengths=lens)
    for name in ("level_db", "activity", "rms_db", "peak", "counts", "flags"):
        assert torch.equal(getattr(a, name), getattr(b2, name)), name
    for b, r in enumerate(rows):
        solo = lv.speech_level(torch.from_numpy(r).cuda(), fs)
        for name in ("level_db", "activity", "rms_db", "peak", "counts", "flags"):
            assert torch.equal(getattr(a, name)[b], getattr(solo, name)[0]), (b, name)


def test_refused_arguments_leave_the_outputs_untouched(lib):
    B, L = 2, 300
    x = torch.rand(B, L, device="cuda")
    lens = torch.tensor([L, 17], dtype=torch.int32, device="cuda")
    ref = torch.ones(B, dtype=torch.float64, device="cuda")
    off = torch.zeros(B, dtype=torch.float64, device="cuda")
    klass = torch.full((B, L), CANARY, dtype=torch.uint8, device="cuda")
    sq = torch.full((B,), SENTINEL, dtype=torch.float64, device="cuda")
    counts = torch.full((B, 16), -1, dtype=torch.int64, device="cuda")
    stats = torch.full((B, 2), SENTINEL, dtype=torch.float64, device="cuda")
    ws = torch.zeros(1024, dtype=torch.float64, device="cuda")
    st = _lib.stream_ptr()

    def dev(v, dtype):
        return torch.tensor(v, dtype=dtype, device="cuda")

    good = dict(x=x.data_ptr(), ldx=L, lens=lens.data_ptr(), off=off.data_ptr(), ref=ref.data_ptr(), B=B, fs=1000.0, tc=0.03, klass=klass.data_ptr(), ldk=L,
                sq=sq.data_ptr(), ws=ws.data_ptr(), nbytes=8192)
    keep = [dev([L + 1, 17], torch.int32), dev([-1, 17], torch.int32)] + [dev([1.0, v], torch.float64) for v in (0.0, -1.0, float("nan"), float("inf"))]
    bad = [dict(x=None), dict(lens=None), dict(ref=None), dict(klass=None), dict(sq=None), dict(ws=None), dict(B=0), dict(B=-1), dict(ldx=L - 1), dict(ldk=L - 1),
           dict(ldk=0), dict(fs=0.0), dict(fs=-8000.0), dict(fs=float("nan")), dict(tc=0.0), dict(tc=-0.03), dict(nbytes=8), dict(lens=keep[0].data_ptr()),
           dict(lens=keep[1].data_ptr())] + [dict(ref=t.data_ptr()) for t in keep[2:]] + [dict(off=keep[4].data_ptr())]
    for change in bad:
        a = dict(good, **change)
        rc = lib.buddy_level_classes(a["x"], a["ldx"], a["lens"], a["off"], a["ref"], a["B"], a["fs"], a["tc"], a["klass"], a["ldk"], a["sq"], a["ws"], a["nbytes"], st)
        assert rc == 2, (change, rc)
    good = dict(klass=klass.data_ptr(), ldk=L, lens=lens.data_ptr(), B=B, I=5, counts=counts.data_ptr(), ws=ws.data_ptr(), nbytes=8192)
    for change in (dict(klass=None), dict(lens=None), dict(counts=None), dict(ws=None), dict(B=0), dict(ldk=L - 1), dict(I=-1), dict(nbytes=8),
                   dict(lens=keep[0].data_ptr())):
        a = dict(good, **change)
        rc = lib.buddy_level_counts(a["klass"], a["ldk"], a["lens"], a["B"], a["I"], a["counts"], a["ws"], a["nbytes"], st)
        assert rc == 2, (change, rc)
    good = dict(x=x.data_ptr(), ldx=L, lens=lens.data_ptr(), B=B, out=stats.data_ptr(), ws=ws.data_ptr(), nbytes=8192)
    for change in (dict(x=None), dict(lens=None), dict(out=None), dict(ws=None), dict(B=0), dict(ldx=L - 1), dict(nbytes=8)):
        a = dict(good, **change)
        rc = lib.buddy_level_stats(a["x"], a["ldx"], a["lens"], a["B"], a["out"], a["ws"], a["nbytes"], st)
        assert rc == 2, (change, rc)
    torch.cuda.synchronize()
    assert (klass == CANARY).all() and (sq == SENTINEL).all() and (counts == -1).all() and (stats == SENTINEL).all()
    for q in (lib.buddy_level_stats_workspace, lib.buddy_level_classes_workspace, lib.buddy_level_counts_workspace):
        assert q(0, 100) == -1 and q(1, -1) == -1 and q(1, 2 ** 30 + 1) == -1 and q(2, 0) > 0
    assert lib.buddy_level_tile() >= 256 and lib.buddy_level_counts_tile() >= 256


# ---- the real-recordings mode -------------------------------------------------------------------------------------------------------------------
MODE = "real_blind_dereverberation"
OVERRIDES = ["tester.sampling_params.T=3", "tester.posterior_sampling.blind_hp.op_updates_per_step=2",
             "tester.posterior_sampling.warm_initialization.mode=reverb_scaled", "tester.real_recordings.chunk_seconds=1.024",
             "tester.real_recordings.overlap_seconds=0.128", "network.nf=32", "tester.sub_batches=1", "tester.overriden_name=run",
             "tester.posterior_sampling.constraint_speech_magnitude.use=false"]
SPEECH, PAUSES = 19200, {"A": 8000, "B": 24000, "C": 64000}      # samples at 16 kHz: the same speech, then a pause of low noise (longer than hangover and fall)


@pytest.fixture(scope="module")
def wavs(tmp_path_factory):
    root = tmp_path_factory.mktemp("level_wavs")
    speech = R.speechlike(41, SPEECH, 16000, pause=0.2).astype(np.float64)
    rs = np.random.RandomState(9)
    for name, pause in PAUSES.items():
        y = np.concatenate([speech, np.zeros(pause)]) + 1e-5 * rs.standard_normal(SPEECH + pause)
        wavfile.write(root / f"{name}.wav", 16000, y.astype(np.float32))
    clicks = 1e-6 * rs.standard_normal(20000)
    clicks[::400] = 0.5                                 # no speech: near silence with clicks, a crest factor the meter flags (EDGE)
    wavfile.write(root / "D.wav", 16000, clicks.astype(np.float32))
    return str(root)


@pytest.fixture(scope="module")
def net():
    from buddy_amd.config import compose
    from buddy_amd.instantiate import instantiate
    from buddy_amd.synth import synth_state_dict
    n = instantiate(compose(tester="real_dereverberation_BUDDy", overrides=OVERRIDES).network)
    n.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(3, 32).items()})
    return n.cuda().eval()


def _run(net, data, out, extra):
    """the mode with the sampler replaced by the identity (what is under test is the scaling in front of it) -> (tester, the mode's directory)"""
    from buddy_amd.config import compose
    from buddy_amd.datasets.recordings import AudioFolder
    from buddy_amd.instantiate import instantiate
    from buddy_amd.testing.tester import Tester
    args = compose(tester="real_dereverberation_BUDDy", overrides=OVERRIDES + [f"model_dir={out}"] + list(extra))
    t = Tester(args, net, instantiate(args.diff_params), test_set=AudioFolder(path=data), device="cuda", in_training=False, batch_size=4)
    t.sampled = 0

    def identity(y, operator, shape=None, blind=False, **kw):
        t.sampler.operator = operator
        t.sampled += 1
        return y.clone()

    t.sampler.predict_conditional = identity
    t.prepare_directories(MODE)
    t.test_real_recordings(MODE)
    return t, t.paths[MODE]


def _degraded_active_rms(base):
    out = {}
    for name in PAUSES:
        sr, a = wavfile.read(os.path.join(base, "degraded", name + ".wav"))
        res = lv.speech_level(torch.from_numpy(a).cuda(), sr)
        assert int(res.flags[0]) == 0
        out[name] = float(res.active_rms[0])
    return out


def test_tester_active_level(net, wavs, tmp_path, capsys):
    """three files of the same speech and 29 %, 56 % and 77 % pause: under ``level: active`` what reaches the network has ONE active level,
    gain scaling_factor / sqrt(reference_activity); under ``std`` it follows the pause share.  Tolerance of the re-measured wavs: they are g y
    rounded to fp32 (2^-24 per sample), and a rounding can flip single threshold decisions: m flipped samples among a >= 16 000 active ones move the
    level by (10 / ln 10) (m / a) (1 + cond) dB; with m <= 8 and cond <= 3 that is below 0.009 dB, 1e-3 of the rms."""
    t, base = _run(net, wavs, str(tmp_path / "a"), ["tester.real_recordings.level=active", "tester.real_recordings.reference_activity=0.5"])
    printed = capsys.readouterr().out
    assert "D.wav: the active level is flagged EDGE: scaled by its std instead" in printed
    target = 0.05 / math.sqrt(0.5)
    rows = {r["file"]: r for r in t.levels}
    assert sorted(rows) == ["A", "B", "C", "D"] and rows["D"]["rule"] == "std" and rows["D"]["flags"] == "EDGE"
    for name in PAUSES:
        r = rows[name]
        assert r["rule"] == "active" and r["flags"] == ""
        assert r["g"] * 10.0 ** (r["level_db"] / 20.0) == pytest.approx(target, rel=1e-12)
    assert rows["A"]["activity"] > rows["B"]["activity"] > rows["C"]["activity"]
    got = _degraded_active_rms(base)
    print("active:", got, "target", target)
    for name in PAUSES:
        assert got[name] == pytest.approx(target, rel=1e-3)
    sr, d = wavfile.read(os.path.join(base, "degraded", "D.wav"))
    assert float(np.std(d.astype(np.float64), ddof=1)) == pytest.approx(0.05, rel=1e-5)
    # the report, and a second run
    with open(os.path.join(base, "levels.csv"), "rb") as f:
        first = f.read()
    assert first.splitlines()[0] == b"file,samples,level_db,activity,rms_db,peak,flags,rule,g" and len(first.splitlines()) == 5
    _, base2 = _run(net, wavs, str(tmp_path / "b"), ["tester.real_recordings.level=active", "tester.real_recordings.reference_activity=0.5"])
    with open(os.path.join(base2, "levels.csv"), "rb") as f:
        assert f.read() == first
    # the std rule on the same files: the speech reaches the network at levels that differ by the constructed amount
    _, base3 = _run(net, wavs, str(tmp_path / "c"), [])
    std = _degraded_active_rms(base3)
    print("std:", std)
    for name in ("B", "C"):
        want = math.sqrt((SPEECH + PAUSES[name]) / (SPEECH + PAUSES["A"]))      # the whole-file rms falls with the pause, the scale rises
        assert std[name] / std["A"] == pytest.approx(want, rel=1e-2)
    assert not os.path.exists(os.path.join(base3, "levels.csv"))


def test_tester_std_makes_no_call_and_writes_the_same_bytes(net, wavs, tmp_path, monkeypatch):
    """``level: std``, the default: with the meter and its three entries made to raise, the mode runs, writes no levels.csv, and every degraded wav
    is byte for byte gain scaling_factor y / std(y)"""
    from buddy_amd.utils.resample import resample

    def boom(*a, **k):
        raise AssertionError("level: std must not touch the meter")

    lib = _lib.load()
    for name in ("buddy_level_stats", "buddy_level_classes", "buddy_level_counts"):
        monkeypatch.setattr(lib, name, boom, raising=False)
    monkeypatch.setattr(lv, "speech_level", boom)
    t, base = _run(net, wavs, str(tmp_path / "s"), ["tester.real_recordings.level=std"])
    assert t.levels is None and not os.path.exists(os.path.join(base, "levels.csv"))
    assert sorted(os.listdir(base)) == ["degraded", "estimated_rir", "reconstructed"]
    for name in list(PAUSES) + ["D"]:
        fs, a = wavfile.read(os.path.join(wavs, name + ".wav"))
        y = resample(torch.from_numpy(np.asarray(a.astype(np.float64))).float().cuda(), fs, 16000)
        want = (1.0 * 0.05 / float(y.std())) * y
        sr, d = wavfile.read(os.path.join(base, "degraded", name + ".wav"))
        assert sr == 16000 and d.tobytes() == want.cpu().numpy().astype(np.float32).tobytes()


def test_tester_active_without_reference_activity_stops_before_sampling(net, wavs, tmp_path):
    from buddy_amd.config import compose
    from buddy_amd.datasets.recordings import AudioFolder
    from buddy_amd.instantiate import instantiate
    from buddy_amd.testing.tester import Tester
    args = compose(tester="real_dereverberation_BUDDy", overrides=OVERRIDES + [f"model_dir={tmp_path}", "tester.real_recordings.level=active"])
    t = Tester(args, net, instantiate(args.diff_params), test_set=AudioFolder(path=wavs), device="cuda", in_training=True, batch_size=4)
    calls = []
    t.sampler.predict_conditional = lambda *a, **k: calls.append(1)
    with pytest.raises(ValueError, match=r"reference_activity.*tools/speech_level\.py --segment-seconds"):
        t.test_real_recordings(MODE)
    assert calls == []
