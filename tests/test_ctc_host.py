"""CPU-side checks of las_ctc_loss / las_ctc_workspace_bytes: sizes are pure host arithmetic, and every bad argument is refused
before anything is launched (no GPU needed: the checks run before the first kernel)."""
import ctypes

import pytest

from test_cabi_and_host import libpath  # noqa: F401  (builds the library)


def _call(l, **kw):
    a = dict(logits=8, sb=10 * 31, st=31, Vc=31, y=8, ldy=6, U=6, enc_len=8, B=2, Tp=10, drop=-1, nll=8, loss=8, scale=8,
             grad=None, gdt=0, gsb=10 * 31, gst=31, ws=8, ws_bytes=1 << 30)
    a.update(kw)
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    return l.las_ctc_loss(p(a["logits"]), a["sb"], a["st"], a["Vc"], p(a["y"]), a["ldy"], a["U"], p(a["enc_len"]), a["B"], a["Tp"],
                          a["drop"], p(a["nll"]), p(a["loss"]), p(a["scale"]), p(a["grad"]), a["gdt"], a["gsb"], a["gst"], p(a["ws"]),
                          a["ws_bytes"], None)


def test_workspace_bytes_is_host_arithmetic(libpath):  # noqa: F811
    from las import _hip
    l = _hip.lib()
    n = l.las_ctc_workspace_bytes(48, 319, 200)
    assert n >= 48 * 319 * 401 * 4 + 2 * 48 * 319 * 201 * 4          # alpha + log-probabilities + posteriors
    assert l.las_ctc_workspace_bytes(48, 319, 201) > n
    assert l.las_ctc_workspace_bytes(0, 319, 200) == 0


@pytest.mark.parametrize("kw,msg", [
    (dict(logits=None), b"must be given"),
    (dict(nll=None), b"must be given"),
    (dict(B=0), b"bad sizes"),
    (dict(Vc=1), b"bad sizes"),
    (dict(ldy=5), b"bad sizes"),
    (dict(U=512, ldy=512), b"at most 511"),
    (dict(st=30), b"strides"),
    (dict(drop=2), b"drop_last_row"),
    (dict(drop=-2), b"drop_last_row"),
    (dict(scale=None), b"need scale_ptr"),
    (dict(grad=8, gdt=7), b"grad_dtype"),
    (dict(grad=8, gst=16), b"grad strides"),
    (dict(ws_bytes=64), b"workspace too small"),
    (dict(ws=None), b"workspace too small"),
])
def test_bad_arguments_are_refused_before_launch(libpath, kw, msg):  # noqa: F811
    from las import _hip
    l = _hip.lib()
    rc = _call(l, **kw)
    assert rc < 0 and msg in l.las_last_error(), l.las_last_error()
