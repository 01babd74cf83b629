"""The extension library libdet6d_hip_ext.so without a GPU: its export table is include/det6d_ext.h both ways, its code
object is gfx950 only, bad arguments return -1 with a message before anything is launched, and its samplers hold
everything in registers / LDS."""
import ctypes
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ext_path():
    from de6d_amd import _build
    _build.build()
    return _build.EXT_LIB


def declared():
    text = open(os.path.join(ROOT, 'include', 'det6d_ext.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(det6d_ext_[a-z0-9_]+)\s*\(', text)))


def test_export_table_equals_the_header_both_ways(ext_path):
    out = subprocess.run(['nm', '-D', '--defined-only', ext_path], capture_output=True, text=True, check=True).stdout
    ours = sorted(line.split()[-1] for line in out.splitlines()
                  if line.split() and line.split()[-2] in ('T', 'W', 'D', 'B') and line.split()[-1].startswith('det6d'))
    assert ours == declared(), set(ours) ^ set(declared())
    from de6d_amd import _lib
    assert _lib.EXT_EXPORTED_SYMBOLS == declared()


def test_code_object_is_gfx950_only(ext_path):
    out = subprocess.run(['strings', ext_path], capture_output=True, text=True).stdout
    assert set(re.findall(r'amdgcn-amd-amdhsa--(gfx[0-9a-f]+)', out)) == {'gfx950'}
    assert 'sm_' not in out and 'nvptx' not in out


def test_bad_arguments_return_minus_one(ext_path):
    import torch  # noqa: F401  (libamdhip64 first, like the product)
    from de6d_amd import _lib
    lib = _lib.ext_lib()
    buf = ctypes.create_string_buffer(1 << 16)
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)
    ws = lib.det6d_ext_fps_features_workspace_bytes(1, 64)
    assert ws >= 64 * 8
    f = lib.det6d_ext_fps_features
    good = [1, 64, 0, 64, 8, p, 8, 4, 1.0, p, ws, p, 8, 0, 0, None]

    def call(**kw):
        names = ['b', 'n_total', 'lo', 'hi', 'm', 'rows', 'ld', 'c', 'gamma', 'ws', 'ws_bytes', 'idx', 'idx_stride',
                 'idx_offset', 'idx_bias', 'stream']
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return f(*args)
    for bad in (dict(hi=65), dict(lo=64), dict(n_total=20000, hi=20000), dict(c=257, ld=260), dict(ld=6), dict(ld=10),
                dict(idx_stride=7), dict(ws_bytes=ws - 1), dict(rows=None), dict(m=-1), dict(c=-1),
                dict(rows=ctypes.c_void_p(p.value + 4))):
        assert call(**bad) == -1, bad
        assert lib.det6d_ext_last_error().startswith(b"det6d_ext_fps_features"), bad
    m = lib.det6d_ext_fps_matrix
    assert m(1, 0, 1, p, p, p, None) == -1
    assert m(1, 16385, 1, p, p, p, None) == -1
    assert m(1, 64, -1, p, p, p, None) == -1
    assert m(1, 64, 4, None, p, p, None) == -1
    assert call(m=0) == 0 and call(b=0) == 0            # nothing to do: nothing launched
    assert lib.det6d_ext_version().startswith(b"det6d-hip-ext gfx950")


def test_samplers_hold_no_scratch_and_spill_nothing(ext_path):
    with open(ext_path.replace('.so', '.usage.json')) as fh:
        usage = {k: u for kernels in json.load(fh).values() for k, u in kernels.items()}
    samplers = {k: u for k, u in usage.items() if 'ffps_features_kernel' in k or 'ffps_matrix_kernel' in k}
    assert len(samplers) == 10, sorted(usage)
    for name, u in samplers.items():
        assert not u.get('ScratchSize') and not u.get('VGPRs Spill') and u.get('Dynamic Stack') != 'True', (name, u)
        assert u['VGPRs'] + u.get('AGPRs', 0) <= 128, (name, u)          # 1024-thread workgroups

