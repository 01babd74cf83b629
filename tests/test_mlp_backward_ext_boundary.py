"""The MLP-backward entry points of libdet6d_hip_ext.so without a GPU: they are declared and exported, every bad argument
returns -1 with a message naming the entry point before anything is launched, the workspace function is monotone and 16-byte
granular, and the kernels hold everything in registers / LDS."""
import ctypes
import json
import os

import pytest

ENTRIES = ('det6d_ext_linear_backward', 'det6d_ext_linear_backward_workspace_bytes')
NAMES = ['rows', 'k', 'n', 'x', 'ldx', 'xcol0', 'w', 'ldw', 'wrow0', 'dz', 'lddz', 'flags', 'dx', 'lddx', 'dxcol0', 'dw', 'lddw',
         'dshift', 'workspace', 'ws_bytes', 'stream']
SLAB = 256


@pytest.fixture(scope="module")
def ext_path():
    from de6d_amd import _build
    _build.build()
    return _build.EXT_LIB


@pytest.fixture(scope="module")
def lib(ext_path):
    import torch  # noqa: F401  (libamdhip64 first, like the product)
    from de6d_amd import _lib
    return _lib.ext_lib()


@pytest.fixture(scope="module")
def p():
    buf = ctypes.create_string_buffer(1 << 16)
    ptr = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)
    ptr._keep = buf
    return ptr


def test_the_entry_points_are_declared_and_loaded(lib):
    from de6d_amd import _lib
    from de6d_amd.ops import mlp_backward
    from tests.test_ext_boundary import declared
    for name in ENTRIES:
        assert name in _lib.EXT_EXPORTED_SYMBOLS and name in declared()
        assert hasattr(lib, name)
    assert lib.det6d_ext_linear_backward.restype is ctypes.c_int
    assert lib.det6d_ext_linear_backward_workspace_bytes.restype is ctypes.c_int64
    assert len(_lib._EXT_SIGNATURES['det6d_ext_linear_backward']) == len(NAMES)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'det6d_ext.h')).read()
    assert 'DET6D_EXT_LINEAR_BACKWARD_SLAB = %d' % mlp_backward.SLAB in header and mlp_backward.SLAB == SLAB
    assert (mlp_backward.RELU_INPUT, mlp_backward.ACCUMULATE_DX) == (1, 2)
    assert lib.det6d_ext_version() == b"det6d-hip-ext gfx950 ext3"


def test_workspace_bytes(lib):
    ws = lib.det6d_ext_linear_backward_workspace_bytes
    for bad in ((-1, 8, 8), ((1 << 24) + 1, 8, 8), (64, 0, 8), (64, 4097, 8), (64, 8, 0), (64, 8, 4097)):
        assert ws(*bad) == -1, bad
    for k, n in ((1, 1), (36, 3), (128, 32), (1536, 512), (4096, 4096)):
        last = 0
        for rows in (0, 1, SLAB, SLAB + 1, 2 * SLAB, 2 * SLAB + 7, 2048, 20480, 1 << 24):
            b = ws(rows, k, n)
            assert b >= last and b % 16 == 0, (rows, k, n)                # monotone in the rows, 16-byte granular
            slabs = -(-rows // SLAB)
            if slabs > 1:
                assert slabs * (k * n + n) * 4 <= b < slabs * (k * n + n) * 4 + 16
            last = b
    assert ws(2048, 512, 128) <= ws(2048, 512, 129) <= ws(2048, 513, 129)  # and in the widths


def test_bad_arguments_return_minus_one(lib, p):
    rows, k, n = 300, 36, 8
    ws = lib.det6d_ext_linear_backward_workspace_bytes(rows, k, n)
    assert ws > 0
    good = [rows, k, n, p, 40, 4, p, 8, 2, p, 8, 3, p, 40, 4, p, 8, p, p, ws, None]
    f = lib.det6d_ext_linear_backward

    def call(**kw):
        args = list(good)
        for key, v in kw.items():
            args[NAMES.index(key)] = v
        return f(*args)
    off4 = ctypes.c_void_p(p.value + 4)
    off2 = ctypes.c_void_p(p.value + 2)
    bad_cases = [dict(rows=-1), dict(rows=(1 << 24) + 1), dict(k=0), dict(k=4097, ldx=8192, lddx=8192), dict(n=0),
                 dict(n=4097, ldw=8192, lddz=8192, lddw=8192), dict(flags=-1), dict(flags=4),
                 dict(dx=None, dw=None, dshift=None), dict(dx=None, flags=2), dict(dx=None, flags=3),
                 dict(ldx=42), dict(ldx=36), dict(xcol0=-1), dict(xcol0=5), dict(ldw=10), dict(ldw=4), dict(wrow0=-1),
                 dict(lddz=7), dict(lddx=39), dict(dxcol0=-1), dict(dxcol0=5), dict(lddw=7),
                 dict(x=off4), dict(w=off4), dict(dz=off2), dict(dx=off2), dict(dw=off2), dict(dshift=off2),
                 dict(ws_bytes=ws - 1), dict(ws_bytes=-1), dict(workspace=None),
                 dict(x=None), dict(w=None), dict(dz=None)]
    for bad in bad_cases:
        assert call(**bad) == -1, bad
        assert lib.det6d_ext_last_error().startswith(b"det6d_ext_linear_backward"), bad
    # x is checked only where it is read: dx alone without the mask takes any x
    assert call(rows=0, dw=None, dshift=None, flags=0, x=None, ldx=0) == 0
    # nothing to do: nothing launched (a launch would fail on a machine without a GPU and could not return 0 there)
    assert call(rows=0, dw=None, dshift=None) == 0
    assert call(rows=0, dw=None, dshift=None, x=None, w=None, dz=None, workspace=None, ws_bytes=0) == 0
    assert call(rows=0, dw=None, dshift=None, flags=2) == 0            # ACCUMULATE_DX onto no rows: dx is left alone


def test_the_kernels_hold_no_scratch_and_spill_nothing(ext_path):
    with open(ext_path.replace('.so', '.usage.json')) as fh:
        usage = json.load(fh)['mlp_backward.hip']
    wanted = ('linear_backward_dx_kernel', 'linear_backward_dw_kernel', 'linear_backward_dshift_kernel',
              'linear_backward_sum_kernel')
    assert all(any(w in k for k in usage) for w in wanted) and all(any(w in k for w in wanted) for k in usage), sorted(usage)
    for name, u in usage.items():
        assert 'ffps_features_kernel' not in name and 'ffps_matrix_kernel' not in name
        assert not u.get('ScratchSize') and not u.get('VGPRs Spill') and not u.get('SGPRs Spill'), (name, u)
        assert u.get('Dynamic Stack') != 'True', (name, u)
        assert u['VGPRs'] + u.get('AGPRs', 0) <= 128, (name, u)            # at least 4 waves per SIMD
        assert u.get('LDS Size', 0) <= 20 * 1024, (name, u)                # several workgroups per CU
