"""Host: the entries of the small network kernels (csrc/capi.hip: buddy_conv_c2in ... buddy_axpy) are declared, bound and exported, and each refuses
with BUDDY_ERR_ARG and a message, before any launch, a null required pointer, an empty shape and every shape its kernels cannot compute.  Nothing
here launches anything: every call below is refused (the pointers are small integers that are never dereferenced)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 2
X, Y, Z, Q = 64, 128, 192, 256          # stand-ins for non-null device pointers
NEW = ("buddy_conv_c2in", "buddy_conv_c2out", "buddy_reflect_pad", "buddy_ola", "buddy_ola_adj", "buddy_unpad_adj", "buddy_pool2", "buddy_up2_acc",
       "buddy_fourier", "buddy_linear", "buddy_softmax_rows", "buddy_softmax_bwd_rows", "buddy_transpose_sq", "buddy_mix2", "buddy_axpy")


@pytest.fixture(scope="module")
def lib():
    from buddy_amd import _lib
    return _lib.load()


def test_err_arg_value():
    hdr = open(os.path.join(ROOT, "buddy_amd", "csrc", "common.h")).read()
    m = re.search(r"#define\s+BUDDY_ERR_ARG\s+(\d+)", hdr)
    assert m and int(m.group(1)) == ERR_ARG


def test_symbols_declared_bound_and_exported(lib):
    from buddy_amd import _lib
    for s in NEW:                                 # header, signatures and exports agree for every name: tests/test_abi_host.py
        assert s in _lib.EXPORTED and hasattr(lib, s), s


def refused(lib, rc):
    return rc == ERR_ARG and len(lib.buddy_last_error()) > 0


def test_conv_c2in_refusals(lib):
    f = lambda x=X, w=Y, add=None, add_ld=0, y=Z, ldY=32, B=2, H=3, W=4, Cout=32, taps=9: \
        lib.buddy_conv_c2in(x, w, None, add, add_ld, y, ldY, B, H, W, Cout, taps, 0, None)
    for kw in (dict(x=None), dict(w=None), dict(y=None), dict(B=0), dict(H=0), dict(W=0), dict(Cout=0), dict(taps=3),
               dict(Cout=30, ldY=32), dict(ldY=28), dict(ldY=34), dict(add=Q, add_ld=28), dict(add=Q, add_ld=34)):
        assert refused(lib, f(**kw)), kw


def test_conv_c2out_refusals(lib):
    f = lambda x=X, ldX=32, w=Y, up=None, y=Z, B=2, H=4, W=4, Cin=32, taps=9, form=-1: \
        lib.buddy_conv_c2out(x, ldX, w, None, up, y, B, H, W, Cin, taps, 0, form, None)
    for kw in (dict(x=None), dict(w=None), dict(y=None), dict(B=0), dict(H=0), dict(W=0), dict(Cin=0), dict(taps=2), dict(Cin=30),
               dict(ldX=28), dict(ldX=34), dict(up=Q, H=3), dict(up=Q, W=5), dict(form=3), dict(form=-2), dict(form=1, taps=1),
               dict(form=2, Cin=16, ldX=16)):
        assert refused(lib, f(**kw)), kw


def test_stft_glue_refusals(lib):
    rp = lambda x=X, xp=Y, B=2, L=20, pad=8, Lp=40: lib.buddy_reflect_pad(x, xp, B, L, pad, Lp, 1.0, None, None)
    for kw in (dict(x=None), dict(xp=None), dict(B=0), dict(L=0), dict(pad=-1), dict(pad=20), dict(Lp=35)):
        assert refused(lib, rp(**kw)), kw
    ola = lambda fr=X, ldF=16, Tp=16, n_fft=16, hop=4, inv=Y, y=Z, B=2, L=20, pad=8, xin=None, ck=None, co=None: \
        lib.buddy_ola(fr, ldF, Tp, n_fft, hop, inv, y, B, L, pad, xin, ck, co, None)
    for kw in (dict(fr=None), dict(inv=None), dict(y=None), dict(B=0), dict(L=0), dict(Tp=0), dict(hop=0), dict(n_fft=0), dict(ldF=15),
               dict(xin=Q), dict(xin=Q, ck=Q), dict(L=70)):
        assert refused(lib, ola(**kw)), kw
    adj = lambda g=X, B=2, L=20, pad=8, Tp=16, n_fft=16, hop=4, inv=Y, fr=Z, ldF=16: lib.buddy_ola_adj(g, B, L, pad, Tp, n_fft, hop, inv, None, fr, ldF, None)
    for kw in (dict(g=None), dict(inv=None), dict(fr=None), dict(B=0), dict(L=0), dict(Tp=0), dict(hop=0), dict(ldF=15)):
        assert refused(lib, adj(**kw)), kw
    un = lambda df=X, ldF=16, T=6, n_fft=16, hop=4, B=2, L=20, pad=8, go=None, ck=None, dx=Z: \
        lib.buddy_unpad_adj(df, ldF, T, n_fft, hop, B, L, pad, 1.0, None, go, ck, dx, None)
    for kw in (dict(df=None), dict(dx=None), dict(B=0), dict(L=0), dict(T=0), dict(hop=0), dict(ldF=15), dict(pad=20), dict(go=Q)):
        assert refused(lib, un(**kw)), kw


def test_pool_and_upsample_refusals(lib):
    pool = lambda s=X, d=Y, B=2, H=4, W=6, C=4: lib.buddy_pool2(s, d, B, H, W, C, 1.0, 0, None)
    for kw in (dict(s=None), dict(d=None), dict(B=0), dict(H=0), dict(C=0), dict(H=3), dict(W=5), dict(C=6), dict(C=3)):
        assert refused(lib, pool(**kw)), kw
    up = lambda s=X, d=Y, B=2, Hs=2, Ws=3, C=4: lib.buddy_up2_acc(s, d, B, Hs, Ws, C, 1.0, 0, None)
    for kw in (dict(s=None), dict(d=None), dict(B=0), dict(Hs=0), dict(Ws=0), dict(C=0), dict(C=3)):
        assert refused(lib, up(**kw)), kw
    # up_add of conv_c2out is the other place that halves H and W
    assert refused(lib, lib.buddy_conv_c2out(X, 32, Y, None, Q, Z, 1, 5, 4, 32, 9, 0, 0, None))


def test_embedding_and_attention_refusals(lib):
    assert refused(lib, lib.buddy_fourier(None, Y, Z, 3, 32, None))
    assert refused(lib, lib.buddy_fourier(X, None, Z, 3, 32, None))
    assert refused(lib, lib.buddy_fourier(X, Y, None, 3, 32, None))
    assert refused(lib, lib.buddy_fourier(X, Y, Z, 0, 32, None))
    assert refused(lib, lib.buddy_fourier(X, Y, Z, 3, 0, None))
    lin = lambda x=X, w=Y, y=Z, B=3, K=64, N=5: lib.buddy_linear(x, w, None, y, B, K, N, 0, None)
    for kw in (dict(x=None), dict(w=None), dict(y=None), dict(B=0), dict(K=0), dict(N=0)):
        assert refused(lib, lin(**kw)), kw
    assert refused(lib, lib.buddy_softmax_rows(None, 4, 4, None))
    assert refused(lib, lib.buddy_softmax_rows(X, 0, 4, None))
    assert refused(lib, lib.buddy_softmax_rows(X, 4, 0, None))
    assert refused(lib, lib.buddy_softmax_bwd_rows(None, Y, 4, 4, None))
    assert refused(lib, lib.buddy_softmax_bwd_rows(X, None, 4, 4, None))
    assert refused(lib, lib.buddy_softmax_bwd_rows(X, Y, 0, 4, None))
    assert refused(lib, lib.buddy_softmax_bwd_rows(X, Y, 4, 0, None))
    tr = lambda s=X, d=Y, batch=3, n=32: lib.buddy_transpose_sq(s, d, batch, n, None)
    for kw in (dict(s=None), dict(d=None), dict(batch=0), dict(n=0), dict(n=48), dict(n=31), dict(d=X)):
        assert refused(lib, tr(**kw)), kw


def test_mix2_and_axpy_refusals(lib):
    assert refused(lib, lib.buddy_mix2(None, Y, None, Z, 10, 0, 0, None))
    assert refused(lib, lib.buddy_mix2(X, None, None, Z, 10, 0, 0, None))
    assert refused(lib, lib.buddy_mix2(X, Y, None, None, 10, 0, 0, None))
    assert refused(lib, lib.buddy_mix2(X, Y, None, Z, 0, 0, 0, None))
    assert refused(lib, lib.buddy_axpy(None, Y, 1.0, 8, 0, None))
    assert refused(lib, lib.buddy_axpy(X, None, 1.0, 8, 0, None))
    assert refused(lib, lib.buddy_axpy(X, Y, 1.0, 0, 0, None))
    for n in (1, 5, 1027):
        assert refused(lib, lib.buddy_axpy(X, Y, 1.0, n, 0, None)), n
