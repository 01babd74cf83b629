"""The grouped-MLP backward entry points of libdet6d_hip_ext.so without a GPU: declared, exported and loaded; every bad
argument returns -1 with the entry point's name in det6d_ext_last_error before anything is launched; zero rows return 0; the
kernels hold no scratch and spill nothing."""
import ctypes
import json
import re
import subprocess

import pytest

from tests.test_ext_boundary import declared

NAMES = ("det6d_ext_group_gather", "det6d_ext_group_pool_backward", "det6d_ext_group_centre_grad", "det6d_ext_vote_backward")


@pytest.fixture(scope="module")
def ext_path():
    from de6d_amd import _build
    _build.build()
    return _build.EXT_LIB


def test_declared_exported_and_loaded(ext_path):
    out = subprocess.run(['nm', '-D', '--defined-only', ext_path], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r'\b(det6d_ext_[a-z0-9_]+)\b', out))
    import torch  # noqa: F401  (libamdhip64 first, like the product)
    from de6d_amd import _lib
    lib = _lib.ext_lib()
    for name in NAMES:
        assert name in declared() and name in exported and name in _lib._EXT_SIGNATURES, name
        assert getattr(lib, name).restype is ctypes.c_int
    assert lib.det6d_ext_version() == b"det6d-hip-ext gfx950 ext3"


def test_bad_arguments_return_minus_one(ext_path):
    import torch  # noqa: F401
    from de6d_amd import _lib
    lib = _lib.ext_lib()
    buf = ctypes.create_string_buffer(1 << 16)
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    p, p4, p1 = ctypes.c_void_p(base), ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 2)

    def check(name, names, good, bads, zero):
        fn = getattr(lib, name)

        def call(**kw):
            args = list(good)
            for k, v in kw.items():
                args[names.index(k)] = v
            return fn(*args)
        for bad in bads:
            assert call(**bad) == -1, (name, bad)
            assert lib.det6d_ext_last_error().startswith(name.encode()), (name, bad, lib.det6d_ext_last_error())
        for z in zero:
            assert call(**z) == 0, (name, z)                        # nothing to do: nothing launched

    check("det6d_ext_group_gather",
          ['b', 'n', 'm', 'ns', 'pts', 'ldp', 'k', 'idx', 'ctr', 'ldctr', 'out', 'ldout', 'stream'],
          [2, 40, 5, 8, p, 8, 7, p, p, 3, p, 8, None],
          [dict(b=-1), dict(n=0), dict(m=-1), dict(ns=0), dict(ns=129), dict(b=4096, m=4096, ns=2), dict(k=2), dict(k=4097, ldp=4100, ldout=4100),
           dict(ldp=6), dict(ldctr=2), dict(ldout=4), dict(ldout=10), dict(out=p4), dict(pts=p1), dict(idx=p1), dict(ctr=p1),
           dict(pts=None), dict(idx=None), dict(ctr=None), dict(out=None)],
          [dict(b=0), dict(m=0), dict(b=0, pts=None, idx=None, ctr=None, out=None)])
    check("det6d_ext_group_pool_backward",
          ['groups', 'ns', 'c', 'y', 'ldy', 'cnt', 'g', 'ldg', 'gcol0', 'dz', 'lddz', 'stream'],
          [10, 8, 6, p, 8, p, p, 12, 4, p, 6, None],
          [dict(groups=-1), dict(ns=0), dict(ns=129), dict(groups=1 << 22, ns=8), dict(c=0), dict(c=4097, ldy=4100, ldg=5000, lddz=4100),
           dict(ldy=5), dict(lddz=5), dict(gcol0=-1), dict(gcol0=7), dict(ldg=9), dict(y=p1), dict(cnt=p1), dict(g=p1), dict(dz=p1),
           dict(y=None), dict(cnt=None), dict(g=None), dict(dz=None)],
          [dict(groups=0), dict(groups=0, y=None, cnt=None, g=None, dz=None)])
    check("det6d_ext_group_centre_grad",
          ['groups', 'ns', 'dx', 'lddx', 'dctr', 'lddctr', 'stream'],
          [10, 8, p, 3, p4, 3, None],
          [dict(groups=-1), dict(ns=0), dict(ns=129), dict(groups=1 << 22, ns=8), dict(lddx=2), dict(lddctr=2), dict(dx=p1), dict(dctr=p1),
           dict(dx=None), dict(dctr=None)],
          [dict(groups=0), dict(groups=0, dx=None, dctr=None)])
    check("det6d_ext_vote_backward",
          ['rows', 'off', 'ldoff', 'rx', 'ry', 'rz', 'dvote', 'lddvote', 'doff', 'lddoff', 'stream'],
          [10, p, 4, 3.0, 3.0, 2.0, p, 3, p4, 3, None],
          [dict(rows=-1), dict(rows=(1 << 24) + 1), dict(ldoff=2), dict(lddvote=2), dict(lddoff=2), dict(rx=-1.0), dict(rz=float('nan')),
           dict(off=p1), dict(dvote=p1), dict(doff=p1), dict(off=None), dict(dvote=None), dict(doff=None)],
          [dict(rows=0), dict(rows=0, off=None, dvote=None, doff=None)])


def test_kernels_hold_no_scratch_and_spill_nothing(ext_path):
    with open(ext_path.replace('.so', '.usage.json')) as fh:
        usage = json.load(fh)['group_backward.hip']
    kinds = ('group_gather_kernel', 'group_pool_backward_kernel', 'group_centre_grad_kernel', 'vote_backward_kernel')
    for kind in kinds:
        assert any(kind in k for k in usage), (kind, sorted(usage))
    assert len(usage) == 6, sorted(usage)                            # two gathers, two routings, the centre sum, the clamp mask
    for name, u in usage.items():
        assert not u.get('ScratchSize') and not u.get('VGPRs Spill') and not u.get('SGPRs Spill'), (name, u)
        assert u.get('Dynamic Stack') != 'True' and not u.get('LDS Size'), (name, u)
