"""The 11 process-wide kernel-selection setters of include/cbim_hip.h: documented defaults, "returns the old value",
and each setter's own argument rule.  Runs against whichever library is loaded; no kernel is launched.

CBIM_WGRAD_R32_C16 has no setter; it is observed through cbim_conv3d_wgrad_workspace, which asks
cbim_wgrad_r32_eligible without a launch (a 96 -> 48 layer reserves room for k_wgrad_r32's slabs only while the
switch is on)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import cbim_amd  # noqa: F401
from cbim_amd import _lib


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _child(code, **env_changes):
    """Run `code` in a fresh Python that loads the library with plain ctypes as `h`; returns its stdout."""
    env = dict(os.environ)
    for k in ("CBIM_CONV_RW48", "CBIM_WGRAD_R32_C16"):
        env.pop(k, None)
    env.update(env_changes)
    src = "import ctypes as C\nh = C.CDLL(%r)\n%s" % (_lib.library_path(), code)
    r = subprocess.run([sys.executable, "-c", src], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip()


# ---- v >= 0 sets, v < 0 queries; the value is kept as an int64 -------------------------------------------------
@pytest.mark.parametrize("name", ["cbim_conv_r32_min_voxels", "cbim_up_tile_min_tiles"])
def test_threshold_setters(L, name):
    f = getattr(L, name)
    old = f(-1)
    try:
        assert f(0) == old              # 0 is a value ("any size"), not a query
        assert f(-1) == 0
        assert f(-7) == 0               # every negative argument only queries
        assert f(1 << 40) == 0
        assert f(-1) == 1 << 40
        assert f(4096) == 1 << 40
        assert f(-1) == 4096
    finally:
        f(old)
    assert f(-1) == old


# ---- only 4 or 8 is accepted, anything else queries ------------------------------------------------------------
@pytest.mark.parametrize("name", ["cbim_conv_r32_tile_depth", "cbim_wgrad_r32_waves"])
def test_four_or_eight_setters(L, name):
    f = getattr(L, name)
    old = f(-1)
    assert old in (4, 8)
    try:
        assert f(4) == old
        for q in (-1, 0, 1, 2, 6, 16):
            assert f(q) == 4            # not 4 or 8: query, nothing stored
        assert f(8) == 4
        assert f(0) == 8
        assert f(4) == 8
    finally:
        f(old)
    assert f(-1) == old


# ---- on >= 0 sets to on ? 1 : 0 --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cbim_conv_pw_enable", "cbim_dwconv_lds_enable"])
def test_boolean_setters(L, name):
    f = getattr(L, name)
    old = f(-1)
    try:
        assert f(0) == old
        assert f(-1) == 0
        assert f(-5) == 0
        assert f(5) == 0                # any positive value stores 1
        assert f(-1) == 1
        assert f(0) == 1
    finally:
        f(old)
    assert f(-1) == old


# ---- on >= 0 sets, the value is stored as given ----------------------------------------------------------------
def test_wgrad_r32_enable(L):
    f = L.cbim_wgrad_r32_enable
    old = f(-1)
    try:
        assert f(0) == old
        assert f(-1) == 0
        assert f(3) == 0
        assert f(-1) == 3
    finally:
        f(old)
    assert f(-1) == old


def test_conv_rw48_enable(L):
    f = L.cbim_conv_rw48_enable
    old = f(-1)
    try:
        assert f(2) == old              # 2 = forced (tests)
        assert f(-1) == 2
        assert f(0) == 2
        assert f(-1) == 0
        assert f(7) == 0                # stored as given
        assert f(-2) == 7
    finally:
        f(old)
    assert f(-1) == old


# ---- always set, to on ? 1 : 0 (no query form) -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["cbim_stem_mfma_enable", "cbim_head_mfma_enable"])
def test_always_setting_setters(L, name):
    f = getattr(L, name)
    old = f(1)                          # (the only way to read it)
    try:
        assert f(0) == 1
        assert f(0) == 0
        assert f(-1) == 0               # a negative argument is true: it sets 1, it does not query
        assert f(5) == 1
        assert f(0) == 1
        assert f(1) == 0
    finally:
        f(old)
    assert f(old) == old


# ---- two switches in one call: a negative argument leaves its half unchanged, returns on | wide << 1 ----------
def test_conv_rw_enable(L):
    f = L.cbim_conv_rw_enable
    old = f(-1, -1)
    try:
        assert f(1, 1) == old
        assert f(0, -1) == 1 | 1 << 1
        assert f(-1, -1) == 0 | 1 << 1
        assert f(-1, 2) == 2            # wide is stored as given (2 = forced)
        assert f(-1, -1) == 0 | 2 << 1
        assert f(3, -1) == 4            # on & 1 is stored
        assert f(-1, -1) == 1 | 2 << 1
        assert f(2, 0) == 5
        assert f(-1, -1) == 0
        assert f(1, 1) == 0
    finally:
        f(old & 1, old >> 1)
    assert f(-1, -1) == old


# ---- the documented defaults, in a fresh process (other tests of a session may have moved a switch) ------------
def test_defaults():
    code = """
h.cbim_conv_r32_min_voxels.restype = h.cbim_up_tile_min_tiles.restype = C.c_int64
h.cbim_conv_r32_min_voxels.argtypes = h.cbim_up_tile_min_tiles.argtypes = [C.c_int64]
print(h.cbim_conv_r32_min_voxels(-1), h.cbim_conv_r32_tile_depth(-1), h.cbim_conv_rw_enable(-1, -1), h.cbim_conv_rw48_enable(-1),
      h.cbim_conv_pw_enable(-1), h.cbim_dwconv_lds_enable(-1), h.cbim_wgrad_r32_enable(-1), h.cbim_wgrad_r32_waves(-1),
      h.cbim_stem_mfma_enable(1), h.cbim_head_mfma_enable(1), h.cbim_up_tile_min_tiles(-1))
"""
    assert _child(code).split() == ["262144", "8", "3", "1", "1", "1", "1", "8", "1", "1", "512"]


# ---- the two environment variables, read by a fresh process ----------------------------------------------------
@pytest.mark.parametrize("env,expect", [(None, "1"), ("0", "0"), ("2", "2")])
def test_conv_rw48_environment(env, expect):
    changes = {} if env is None else {"CBIM_CONV_RW48": env}
    assert _child("print(h.cbim_conv_rw48_enable(-1))", **changes) == expect


_WS_CODE = """
class D(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("dtype", "N", "Di", "Hi", "Wi", "Cin", "Do", "Ho", "Wo", "Cout",
                                       "kD", "kH", "kW", "pD", "pH", "pW", "act")]
h.cbim_conv3d_wgrad_workspace.restype = C.c_size_t
h.cbim_conv3d_wgrad_workspace.argtypes = [C.POINTER(D)]
def ws(ci, co):
    d = D(1, 1, 128, 128, 128, ci, 128, 128, 128, co, 3, 3, 3, 1, 1, 1, 0)   # dtype 1 = CBIM_BF16
    return h.cbim_conv3d_wgrad_workspace(C.byref(d))
print(ws(96, 48), ws(96, 64))
"""


def test_wgrad_r32_c16_environment():
    """96 -> 48 @128^3 bf16: with the switch on the query reserves k_wgrad_r32's slabs (larger than k_conv_wgrad's);
    CBIM_WGRAD_R32_C16=0 leaves k_conv_wgrad's size.  96 -> 64 does not depend on the switch."""
    on48, on64 = map(int, _child(_WS_CODE).split())
    off48, off64 = map(int, _child(_WS_CODE, CBIM_WGRAD_R32_C16="0").split())
    one48, one64 = map(int, _child(_WS_CODE, CBIM_WGRAD_R32_C16="1").split())
    assert on64 == off64 == one64
    assert (on48, on64) == (one48, one64)
    assert off48 < on48
