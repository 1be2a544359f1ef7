"""CPU: the host side of the projection SDR report (buddy_amd/utils/sdr.py): the definition checked on the float64 restatement
tests/_sdr_ref.py (lag products against the time-domain construction of bss_eval, three solvers against each other, nested orders, order 1 in closed
form), the CSV writers, the options parser, the tool's argument errors and the shipped configs."""
import importlib.util
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sdr_ref as R  # noqa: E402

from buddy_amd import _lib  # noqa: E402
from buddy_amd.utils import sdr as S  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location("buddy_tools_" + name, os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


@pytest.mark.parametrize("n,m", [(300, 1), (300, 7), (1000, 64), (4000, 512)])
def test_lag_products_equal_time_domain(n, m):
    """without loading, p_m = h^T d from the lag products is the energy of the least-squares projection onto the zero-padded delayed copies (their Gram
    matrix is the Toeplitz matrix of r): the two SDR agree within 1e-8 dB and the two filters are one"""
    rs = np.random.RandomState(n + m)
    x = rs.standard_normal(n)
    e = np.convolve(x, R.decaying_response(5, 200, 0.01))[:n] + 0.1 * rs.standard_normal(n)
    got, _, h = R.evaluate(e, x, (m,), loading=0.0)
    want, hw = R.time_domain(e, x, m)
    print(f"n {n} m {m}: lag products {got[0]:.10f} dB, time domain {want:.10f} dB, filters differ by {np.abs(h - hw).max():.2e}")
    assert abs(got[0] - want) <= 1e-8 and -30.0 < want < 30.0                             # an ordinary value: neither side sits at a floor
    assert np.abs(h - hw).max() <= 1e-9 * np.abs(hw).max()


def test_routes_agree_on_the_gpu_tests_inputs():
    """LU, Cholesky and scipy's solve_toeplitz agree within 1e-6 dB on every pair the GPU tests compare against the restatement, and SDR is
    non-decreasing in the order (nested subspaces) up to that disagreement"""
    cases = [(name, R.solve_case(name), R.ORDERS) for name in R.solve_pairs()] + [("fir40_noise", R.known_case("fir40_noise"), R.TAPS)]
    for name, c, orders in cases:
        print(f"{name}: routes disagree by {c['tol_db']:.2e} dB, {c['tol_h']:.2e} in h; SDR {np.round(c['sdr'], 4).tolist()} at {list(orders)}")
        assert c["tol_db"] <= 1e-6, name
        for route in R.ROUTES:
            v = c["routes"][route][0]
            assert np.all(np.diff(v) >= -c["tol_db"]) and np.all(np.isfinite(v)), (name, route)
        assert c["sdr"][-1] - c["sdr"][0] > 10.0, name               # the curve rises: the inputs have something to forgive


def test_order_one_closed_form():
    """m = 1 is a scale: SDR_1 = 10 log10(<e,x>^2 / (||e||^2 ||x||^2 - <e,x>^2)) up to the loading, whose effect is
    -(10 / ln 10) lambda (1 + 10^(SDR / 10)) dB to first order"""
    for name, (e, x) in R.solve_pairs().items():
        e, x = e.astype(np.float64), x.astype(np.float64)
        ex, ee, xx = e @ x, e @ e, x @ x
        want = 10.0 * math.log10(ex * ex / (ee * xx - ex * ex))
        got = R.evaluate(e, x, (1,))[0][0]
        shift = -(10.0 / math.log(10.0)) * R.LOADING * (1.0 + 10.0 ** (want / 10.0))
        assert abs(got - want - shift) <= 1e-11 and abs(R.evaluate(e, x, (1,), loading=0.0)[0][0] - want) <= 1e-11, name


def test_identical_pair_reads_the_ceiling():
    e, x = R.known_pairs()["same"]
    v, p, h = R.evaluate(e, x, R.TAPS)
    assert np.all(np.abs(v - 90.0) < 0.01) and abs(h[0] - 1.0 / (1.0 + R.LOADING)) < 1e-9 and np.abs(h[1:]).max() < 1e-9


def _evaluation(vals, flags, samples, taps=S.TAPS, alignment=None):
    t = lambda v, dt: torch.as_tensor(v, dtype=dt)
    return S.SdrEvaluation(t(vals, torch.float64), t(flags, torch.int32), t(samples, torch.int32), taps, None, alignment)


def test_csv_round_trip(tmp_path):
    from buddy_amd.utils.metrics import Alignment
    nan = float("nan")
    inp = _evaluation([[-13.5, -2.0, 4.0 / 3.0, 13.25], [nan] * 4], [1, 0], [16000, 1])
    out = _evaluation([[-3.5, 2.0, 8.0 / 3.0, 90.0], [nan] * 4], [3, 0], [16000, 1])
    rows = S.report_rows(["a", "b"], inp, out)
    cols = ["file"] + [f"sdr{m}_{k}" for m in S.TAPS for k in ("in", "out", "delta")] + ["flags_in", "flags_out", "samples"]
    assert list(rows[0]) == cols and out.names == ("sdr1", "sdr64", "sdr512", "sdr2048")
    assert rows[0]["sdr1_delta"] == 10.0 and rows[0]["sdr512_delta"] == 8.0 / 3.0 - 4.0 / 3.0 and math.isnan(rows[1]["sdr64_delta"])
    assert rows[0]["flags_out"] == 3 and rows[1]["samples"] == 1
    p = str(tmp_path / "sdr.csv")
    S.write_report(p, rows)
    assert open(p).read().splitlines()[2] == "b,,,,,,,,,,,,,0,0,1"                      # NaN is an empty field
    back = R.read_csv(p)
    for a, b in zip(rows, back):
        assert list(a) == list(b)
        for k in a:
            assert (isinstance(a[k], float) and math.isnan(a[k]) and math.isnan(b[k])) or a[k] == b[k], k      # repr(float) reads back exactly
    summ = S.summary_rows(rows)
    assert [s["value"] for s in summ] == cols[1:13]
    by = {s["value"]: s for s in summ}
    assert by["sdr2048_out"]["n"] == 1 and by["sdr2048_out"]["mean"] == 90.0 and by["sdr2048_out"]["std"] == 0.0
    assert "sdr512_out" in S.format_summary(summ) and S.summary_rows([]) == []
    blank = S.SdrEvaluation.blank_like(out)
    assert torch.isnan(blank.values).all() and not blank.flags.any() and blank.samples is out.samples and blank.taps == out.taps
    two = S.report_rows(["a"], _evaluation([[1.0, 2.0]], [1], [9], taps=(3, 700)), _evaluation([[2.0, 4.0]], [1], [9], taps=(3, 700)))
    assert list(two[0]) == ["file", "sdr3_in", "sdr3_out", "sdr3_delta", "sdr700_in", "sdr700_out", "sdr700_delta", "flags_in", "flags_out", "samples"]
    out.alignment = Alignment(torch.tensor([3, 0], dtype=torch.int32), torch.tensor([0.75, nan], dtype=torch.float64), torch.tensor([0.125, 0.0], dtype=torch.float64),
                              torch.tensor([1, 0], dtype=torch.int32), None, None, torch.tensor([15997, 1], dtype=torch.int32), 800, 16000)
    lagged = S.report_rows(["a", "b"], inp, out)
    assert list(lagged[0]) == cols + ["lag_in", "lag_out", "lag_ms_in", "lag_ms_out", "xcorr_in", "xcorr_out", "align_flags_in", "align_flags_out"]
    assert lagged[0]["lag_out"] == 3 and math.isnan(lagged[0]["lag_in"])
    assert [s["value"] for s in S.summary_rows(lagged)][12:] == ["lag_ms_in", "lag_ms_out", "xcorr_in", "xcorr_out"]


def test_taps_of():
    assert S.taps_of([512, 1, 64]) == (1, 64, 512) and S.taps_of((2048,)) == (2048,) and S.TAPS == (1, 64, 512, 2048) and S.LOADING == 1e-9
    for bad in ([], [0], [2049], [1, 1], [1.5], list(range(1, 10))):
        with pytest.raises(ValueError, match="taps"):
            S.taps_of(bad)


def test_sdr_options_default_off():
    from buddy_amd.config import compose
    from buddy_amd.testing.tester import sdr_options
    assert sdr_options({}) == (False, S.TAPS)                                             # a config written before the block existed
    assert sdr_options({"sdr": {"use": True}}) == (True, S.TAPS) and sdr_options({"sdr": {}}) == (False, S.TAPS)
    assert sdr_options({"sdr": {"use": True, "taps": [512]}}) == (True, (512,))
    conf = os.path.join(ROOT, "conf", "tester")
    shipped = sorted(f[:-5] for f in os.listdir(conf) if f.endswith(".yaml"))
    for name in shipped:
        assert sdr_options(compose(tester=name).tester) == (False, S.TAPS), name
    for name in ("blind_dereverberation_BUDDy", "informed_dereverberation_DPS"):          # the two paired configs ship the block, switched off
        cfg = compose(tester=name).tester
        assert cfg.sdr.use is False and list(cfg.sdr.taps) == list(S.TAPS), name
        assert sdr_options(compose(tester=name, overrides=["tester.sdr.use=true", "tester.sdr.taps=[1,512]"]).tester) == (True, (1, 512))
    assert compose(tester="real_dereverberation_BUDDy").tester.get("sdr", None) is None   # no clean signal there


def test_sdr_has_no_cpu_form():
    x = torch.zeros(1, 8000)
    with pytest.raises(_lib.BuddyHipError):
        S.evaluate(x, x, 16000)
    lib = _lib.load()
    T, K = lib.buddy_sdr_tile(), lib.buddy_sdr_lag_tile()
    assert T >= K >= 64 and T % K == 0
    assert lib.buddy_sdr_products_workspace(3, 3 * T + 17, 2 * K + 3) == 8 * 3 * 4 * (2 * (2 * K + 3) + 1)
    assert lib.buddy_sdr_products_workspace(3, T, 1) == 8 * 3 * 3 and lib.buddy_sdr_products_workspace(0, T, 1) == -1
    assert lib.buddy_sdr_products_workspace(3, T, 2049) == -1 and lib.buddy_sdr_products_workspace(3, 0, 1) == -1
    assert lib.buddy_sdr_products_workspace(3, 2 ** 30 + 1, 1) == -1


def test_tool_argument_errors(tmp_path, capsys):
    tool = _tool("sdr")
    d = str(tmp_path)
    for argv in (["--reference", d], [d, "--estimate", d], [], ["--reference", d, "--estimate", d, "--taps", "0"],
                 ["--reference", d, "--estimate", d, "--taps", "1", "1"], ["--reference", d, "--estimate", d, "--taps", "4096"],
                 ["--reference", d, "--estimate", d, "--taps", *[str(m) for m in range(1, 10)]], ["--reference", d, "--estimate", d, "--loading", "-1"]):
        with pytest.raises(SystemExit) as ex:
            tool.main(argv)
        assert ex.value.code == 2, argv                                                   # argparse's error exit, before anything is read or scored
    capsys.readouterr()
    with pytest.raises(SystemExit, match="no wav name"):
        tool.main(["--reference", d, "--estimate", d])


def test_compare_knows_the_report():
    assert "sdr" in _tool("compare").REPORTS
