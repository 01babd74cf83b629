"""The c-fps / df-fps entry points of libdet6d_hip_ext.so without a GPU: they are declared and exported, bad arguments return
-1 with a message naming the entry point before anything is launched, and their kernels hold everything in registers / LDS."""
import ctypes
import json

import pytest


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
    for name in ('det6d_ext_topk_scores', 'det6d_ext_pillar_weights'):
        assert name in _lib.EXT_EXPORTED_SYMBOLS
        assert getattr(lib, name).restype is ctypes.c_int


def test_topk_bad_arguments_return_minus_one(lib, p):
    f = lib.det6d_ext_topk_scores
    names = ['b', 'n_total', 'lo', 'hi', 'm', 'scores', 'gamma', 'idx', 'idx_stride', 'idx_offset', 'idx_bias', 'stream']
    good = [1, 64, 0, 64, 8, p, 1.0, p, 8, 0, 0, None]

    def call(**kw):
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return f(*args)
    for bad in (dict(hi=65), dict(lo=64), dict(lo=70, hi=64), dict(lo=-1), dict(n_total=20000, hi=20000), dict(n_total=0),
                dict(m=-1), dict(m=65, idx_stride=100), dict(lo=32, m=33, idx_stride=100), dict(idx_stride=7),
                dict(idx_offset=1), dict(idx_offset=-1), dict(scores=None), dict(idx=None), dict(b=-1)):
        assert call(**bad) == -1, bad
        assert lib.det6d_ext_last_error().startswith(b"det6d_ext_topk_scores"), bad
    assert call(m=0) == 0 and call(b=0) == 0            # nothing to do: nothing launched


def test_pillar_weights_bad_arguments_return_minus_one(lib, p):
    f = lib.det6d_ext_pillar_weights
    names = ['b', 'n_total', 'lo', 'hi', 'xyz', 'weights', 'stream']
    good = [1, 64, 0, 64, p, p, None]

    def call(**kw):
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return f(*args)
    for bad in (dict(hi=65), dict(lo=64), dict(lo=70, hi=64), dict(lo=-1), dict(n_total=20000, hi=20000), dict(n_total=0),
                dict(xyz=None), dict(weights=None), dict(b=-1)):
        assert call(**bad) == -1, bad
        assert lib.det6d_ext_last_error().startswith(b"det6d_ext_pillar_weights"), bad
    assert call(b=0) == 0


def test_sort_kernels_hold_no_scratch_and_spill_nothing(ext_path):
    with open(ext_path.replace('.so', '.usage.json')) as fh:
        usage = json.load(fh)['sort_samplers.hip']
    topk = {k: u for k, u in usage.items() if 'topk_scores_kernel' in k}
    pillars = {k: u for k, u in usage.items() if 'pillar_weights_kernel' in k}
    assert len(topk) == 7 and len(pillars) == 7, sorted(usage)           # 256 .. 16384 entries
    for name, u in {**topk, **pillars}.items():
        assert not u.get('ScratchSize') and not u.get('VGPRs Spill') and not u.get('SGPRs Spill'), (name, u)
        assert u.get('Dynamic Stack') != 'True', (name, u)
        assert u['VGPRs'] + u.get('AGPRs', 0) <= 128, (name, u)          # 1024-thread workgroups
        assert u['LDS Size'] <= 16384 * 8, (name, u)                     # the slice as 64-bit entries, nothing else
    assert max(u['LDS Size'] for u in topk.values()) == 16384 * 8
