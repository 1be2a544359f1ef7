"""gemm = "f16" (the opt-in fast mode of the Winograd-domain GEMMs) on the host side: the option value, its environment word and the Python
constructor.  No GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_option_validate_accepts_gemm_3_only():
    from buddy_amd import _lib
    lib = _lib.load()
    assert lib.buddy_option_validate(b"gemm", 3) == 0
    assert lib.buddy_option_validate(b"gemm", 2) == 0
    assert lib.buddy_option_validate(b"gemm", 4) != 0
    assert lib.buddy_option_validate(b"gemm", -1) != 0


def test_environment_word_f16_loads():
    code = "import sys; sys.path.insert(0, %r); from buddy_amd import _lib; _lib.load(); print('loaded')" % ROOT
    e = {k: v for k, v in os.environ.items() if not k.startswith("BUDDY_")}
    e["BUDDY_GEMM"] = "f16"
    ok = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=e, timeout=300)
    assert ok.returncode == 0 and "loaded" in ok.stdout, ok.stderr[-800:]
    e["BUDDY_GEMM"] = "fp16"
    bad = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=e, timeout=300)
    assert bad.returncode != 0 and "BUDDY_GEMM" in bad.stderr


def test_constructor_accepts_f16_and_refuses_near_misses():
    from buddy_amd.networks.ncsnpp import NCSNppTime
    stft = {"n_fft": 126, "hop_length": 32, "center": True}
    net = NCSNppTime(stft=stft, nf=32, ch_mult=(1, 2), num_res_blocks=1, gemm="f16")
    assert net.gemm == "f16" and NCSNppTime.GEMM_MODES["f16"] == 3
    for bad in ("f16 ", 4):
        with pytest.raises(NotImplementedError):
            NCSNppTime(stft=stft, nf=32, ch_mult=(1, 2), num_res_blocks=1, gemm=bad)
    net.set_option("gemm", 3)
    assert net.replica()._options == {"gemm": 3}


def test_library_sizes_the_f16_image():
    from buddy_amd import _lib
    lib = _lib.load()
    assert lib.buddy_wgemm_f16_packed_bytes(64, 128, 256) == 64 * 128 * 256 * 2 + 512
    assert lib.buddy_wgemm_f16_packed_bytes(64, 96, 256) == 0          # Cout % 128
    assert lib.buddy_wgemm_f16_packed_bytes(65, 128, 256) == 0         # positions <= 64
