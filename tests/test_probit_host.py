"""ob_probit without a GPU: every argument check returns before any device work (no context is
needed to reach them), and probit() is exported."""
import ctypes as C

import numpy as np


def _call(N, x, ldx, y, n, k, beta):
    conv, it = C.c_int32(-1), C.c_int32(-1)
    rc = N.lib().ob_probit(None, x, ldx, y, n, k, 100, 1e-6, beta, C.byref(conv), C.byref(it))
    return rc, N.lib().ob_last_error()


def test_probit_checks_arguments_before_any_device_work(N):
    d = np.ones(64)
    dp = d.ctypes.data_as(C.POINTER(C.c_double))
    for args in ((None, 8, dp, 8, 2, dp), (dp, 8, None, 8, 2, dp), (dp, 8, dp, 8, 2, None)):
        rc, msg = _call(N, *args)
        assert rc == N.OB_E_INVALID and b"null pointer" in msg
    for n in (0, -3):
        rc, msg = _call(N, dp, 8, dp, n, 2, dp)
        assert rc == N.OB_E_INVALID and b"n > 0" in msg
    rc, msg = _call(N, dp, 8, dp, 8, 0, dp)
    assert rc == N.OB_E_INVALID and b"k >= 1" in msg
    rc, msg = _call(N, dp, 1, dp, 1, 33, dp)
    assert rc == N.OB_E_UNSUPPORTED and b"32" in msg
    rc, msg = _call(N, dp, 7, dp, 8, 2, dp)
    assert rc == N.OB_E_INVALID and b"ldx" in msg
    # a valid shape reaches the context check, still without touching a device
    rc, msg = _call(N, dp, 8, dp, 8, 2, dp)
    assert rc == N.OB_E_INVALID and b"ctx" in msg


def test_probit_is_exported(ob, N):
    assert callable(ob.probit) and "probit" in ob.__all__
    assert N.OB_HECKMAN_MAX_ZSEL == 31
