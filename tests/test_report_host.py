"""CPU: the one summary and the one CSV writer behind every evaluation report (buddy_amd/utils/report.py).  Each module's ``summary_rows`` keeps its own
selection of columns; the expected values below are what the four separate implementations returned for these rows before they were folded into
``report.summarise``, written down as literals."""
import math

from buddy_amd.utils import acoustics, level, metrics, report, spectral, srmr

nan = float("nan")

METRICS_ROWS = [
    {"file": "a", "samples": 16000, "si_sdr_in": 1.5, "si_sdr_out": 7.25, "si_sdr_delta": 5.75, "stoi_in": 0.5, "stoi_out": 0.75, "stoi_delta": 0.25,
     "flags_in": 3, "flags_out": 3, "kept_frames": 70, "frames": 77, "lag_in": 3, "lag_out": -2, "lag_ms_in": 0.1875, "lag_ms_out": -0.125,
     "xcorr_in": 0.9, "xcorr_out": 0.95, "align_flags_in": 1, "align_flags_out": 1},
    {"file": "b", "samples": 15000, "si_sdr_in": nan, "si_sdr_out": 3.0, "si_sdr_delta": nan, "stoi_in": 0.25, "stoi_out": nan, "stoi_delta": nan,
     "flags_in": 2, "flags_out": 1, "kept_frames": 0, "frames": 70, "lag_in": 0, "lag_out": 5, "lag_ms_in": 0.0, "lag_ms_out": 0.3125,
     "xcorr_in": nan, "xcorr_out": -0.5, "align_flags_in": 0, "align_flags_out": 5},
    {"file": "c", "samples": 8000, "si_sdr_in": -2.0, "si_sdr_out": 4.5, "si_sdr_delta": 6.5, "stoi_in": 0.625, "stoi_out": 0.875, "stoi_delta": 0.25,
     "flags_in": 3, "flags_out": 3, "kept_frames": 31, "frames": 37, "lag_in": -1, "lag_out": 0, "lag_ms_in": -0.0625, "lag_ms_out": 0.0,
     "xcorr_in": 0.7, "xcorr_out": 0.8, "align_flags_in": 1, "align_flags_out": 3},
]
METRICS_SUMMARY = [
    ("si_sdr_in", 2, -0.25, -0.25, 1.75), ("si_sdr_out", 3, 4.916666666666667, 4.5, 1.7598926734952396), ("si_sdr_delta", 2, 6.125, 6.125, 0.375),
    ("stoi_in", 3, 0.4583333333333333, 0.5, 0.15590239111558088), ("stoi_out", 2, 0.8125, 0.8125, 0.0625), ("stoi_delta", 2, 0.25, 0.25, 0.0),
    ("lag_ms_in", 3, 0.041666666666666664, 0.0, 0.10622957319984969), ("lag_ms_out", 3, 0.0625, 0.0, 0.1839950180484968),
    ("xcorr_in", 2, 0.8, 0.8, 0.10000000000000003), ("xcorr_out", 3, 0.4166666666666667, 0.8, 0.651067499487487),
]

SPECTRAL_ROWS = [
    {"file": "a", "samples": 16000, "cd_in": 4.5, "cd_out": 2.25, "cd_delta": -2.25, "llr_in": 0.75, "llr_out": 0.5, "llr_delta": -0.25,
     "fwsegsnr_in": 3.0, "fwsegsnr_out": 9.5, "fwsegsnr_delta": 6.5, "flags_in": 7, "flags_out": 7, "frames": 98, "llr_frames_in": 90,
     "llr_frames_out": 91, "fwsegsnr_frames_in": 98, "fwsegsnr_frames_out": 98, "lag_in": 3, "lag_out": -2, "lag_ms_in": 0.1875, "lag_ms_out": -0.125,
     "xcorr_in": 0.9, "xcorr_out": 0.95, "align_flags_in": 1, "align_flags_out": 1},
    {"file": "b", "samples": 300, "cd_in": nan, "cd_out": nan, "cd_delta": nan, "llr_in": nan, "llr_out": 1.25, "llr_delta": nan,
     "fwsegsnr_in": nan, "fwsegsnr_out": nan, "fwsegsnr_delta": nan, "flags_in": 0, "flags_out": 2, "frames": 0, "llr_frames_in": 0,
     "llr_frames_out": 1, "fwsegsnr_frames_in": 0, "fwsegsnr_frames_out": 0, "lag_in": 0, "lag_out": 0, "lag_ms_in": nan, "lag_ms_out": 0.0,
     "xcorr_in": nan, "xcorr_out": 0.25, "align_flags_in": 0, "align_flags_out": 3},
    {"file": "c", "samples": 8000, "cd_in": 5.0, "cd_out": 3.5, "cd_delta": -1.5, "llr_in": 1.0, "llr_out": 0.625, "llr_delta": -0.375,
     "fwsegsnr_in": -1.5, "fwsegsnr_out": 6.0, "fwsegsnr_delta": 7.5, "flags_in": 7, "flags_out": 7, "frames": 48, "llr_frames_in": 40,
     "llr_frames_out": 44, "fwsegsnr_frames_in": 48, "fwsegsnr_frames_out": 48, "lag_in": -1, "lag_out": 4, "lag_ms_in": -0.0625, "lag_ms_out": 0.25,
     "xcorr_in": 0.7, "xcorr_out": 0.8, "align_flags_in": 1, "align_flags_out": 1},
]
SPECTRAL_SUMMARY = [
    ("cd_in", 2, 4.75, 4.75, 0.25), ("cd_out", 2, 2.875, 2.875, 0.625), ("cd_delta", 2, -1.875, -1.875, 0.375),
    ("llr_in", 2, 0.875, 0.875, 0.125), ("llr_out", 3, 0.7916666666666666, 0.625, 0.3280836614171588), ("llr_delta", 2, -0.3125, -0.3125, 0.0625),
    ("fwsegsnr_in", 2, 0.75, 0.75, 2.25), ("fwsegsnr_out", 2, 7.75, 7.75, 1.75), ("fwsegsnr_delta", 2, 7.0, 7.0, 0.5),
    ("lag_ms_in", 2, 0.0625, 0.0625, 0.125), ("lag_ms_out", 3, 0.041666666666666664, 0.0, 0.15590239111558088),
    ("xcorr_in", 2, 0.8, 0.8, 0.10000000000000003), ("xcorr_out", 3, 0.6666666666666666, 0.8, 0.3009245014211298),
]

SRMR_ROWS = [
    {"file": "a", "samples_in": 16000, "samples_out": 16000, "srmr_in": 2.5, "srmr_out": 4.0, "srmr_delta": 1.5, "kstar_in": 5, "kstar_out": 6, "bw_in": 35.5,
     "bw_out": 40.25, "flags_in": 1, "flags_out": 1, "frames_in": 12, "frames_out": 12, "srmr_clean": 6.5, "kstar_clean": 7, "bw_clean": 44.0},
    {"file": "b", "samples_in": 3000, "samples_out": 3000, "srmr_in": nan, "srmr_out": nan, "srmr_delta": nan, "kstar_in": 0, "kstar_out": 0, "bw_in": nan,
     "bw_out": nan, "flags_in": 0, "flags_out": 0, "frames_in": 0, "frames_out": 0, "srmr_clean": nan, "kstar_clean": 0, "bw_clean": nan},
    {"file": "c", "samples_in": 20000, "samples_out": 20000, "srmr_in": 3.25, "srmr_out": 3.0, "srmr_delta": -0.25, "kstar_in": 5, "kstar_out": 5, "bw_in": 36.0,
     "bw_out": 36.5, "flags_in": 1, "flags_out": 1, "frames_in": 16, "frames_out": 16, "srmr_clean": 7.0, "kstar_clean": 8, "bw_clean": 50.0},
]
SRMR_SUMMARY = [("srmr_in", 2, 2.875, 2.875, 0.375), ("srmr_out", 2, 3.5, 3.5, 0.5), ("srmr_delta", 2, 0.625, 0.625, 0.875), ("srmr_clean", 2, 6.75, 6.75, 0.25)]

LEVEL_ROWS = [
    {"file": "a", "samples": 16000, "level_db": -20.5, "activity": 0.75, "rms_db": -21.75, "peak": 0.5, "flags": "", "frames": 10},
    {"file": "b", "samples": 0, "level_db": nan, "activity": nan, "rms_db": nan, "peak": 0.0, "flags": "UNDEFINED", "frames": 0},
    {"file": "c", "samples": 8000, "level_db": -30.0, "activity": 0.5, "rms_db": -33.0, "peak": 0.25, "flags": "EDGE", "frames": 5},
    {"file": "d", "samples": 100, "level_db": nan, "activity": nan, "rms_db": -50.0, "peak": 0.01, "flags": "BELOW|UNDEFINED", "frames": 1},
]
LEVEL_SUMMARY = [("level_db", 2, -25.25, -25.25, 4.75), ("activity", 2, 0.625, 0.625, 0.125), ("rms_db-level_db", 2, -2.125, -2.125, 0.875)]


def _same(got, expected):
    assert [s["value"] for s in got] == [e[0] for e in expected]
    for s, (_, n, mean, median, std) in zip(got, expected):
        assert list(s) == ["value", "n", "mean", "median", "std"]
        assert s["n"] == n and s["mean"] == mean and s["median"] == median and s["std"] == std, s


def test_summary_rows_keep_their_columns_and_values():
    _same(metrics.summary_rows(METRICS_ROWS), METRICS_SUMMARY)
    _same(spectral.summary_rows(SPECTRAL_ROWS), SPECTRAL_SUMMARY)
    _same(srmr.summary_rows(SRMR_ROWS), SRMR_SUMMARY)
    _same(level.summary_rows(LEVEL_ROWS), LEVEL_SUMMARY)
    # a generator of rows; no rows: a paired report and the SRMR report have no summary, the level report keeps its three lines with n = 0
    _same(metrics.summary_rows(r for r in METRICS_ROWS), METRICS_SUMMARY)
    assert metrics.summary_rows([]) == spectral.summary_rows([]) == srmr.summary_rows([]) == []
    empty = level.summary_rows([])
    assert [s["value"] for s in empty] == [e[0] for e in LEVEL_SUMMARY] and all(s["n"] == 0 and math.isnan(s["mean"]) and math.isnan(s["std"]) for s in empty)
    assert metrics.write_report is spectral.write_report is srmr.write_report is level.write_report is acoustics.write_report is report.write_report


def test_format_summary_keeps_each_module_widths():
    s = [{"value": "x_out", "n": 7, "mean": 1.5, "median": -2.25, "std": 0.125}]
    tail = "  mean     1.5000  median    -2.2500  std    0.1250"
    assert metrics.format_summary(s) == srmr.format_summary(s) == "         x_out  n    7" + tail
    assert spectral.format_summary(s) == "           x_out  n    7" + tail
    assert level.format_summary(s) == "           x_out  n     7" + tail
    assert metrics.format_summary(s + s) == "\n".join([metrics.format_summary(s)] * 2) and metrics.format_summary([]) == ""
