"""The target-assignment entry points of libdet6d_hip_ext.so without a GPU: they are declared and exported, bad arguments
return -1 with a message naming the entry point before anything is launched, calls with nothing to do launch nothing, and the
kernel holds everything in registers / LDS."""
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


COMMON = ['n_points', 'points', 'ld_points', 'xyz_col', 'bs_col', 'n_per_scene', 'b', 'm', 'boxes', 'ld_boxes', 'extra_width']
BAD_COMMON = (dict(n_points=-1), dict(n_points=(1 << 24) + 1), dict(b=-1), dict(b=4097), dict(m=-1), dict(m=1025),
              dict(ld_points=2, xyz_col=0, bs_col=-1, n_per_scene=64), dict(xyz_col=-1), dict(xyz_col=2), dict(ld_points=1025),
              dict(bs_col=4), dict(bs_col=-1, n_per_scene=0), dict(bs_col=-1, n_per_scene=-5), dict(ld_boxes=8),
              dict(ld_boxes=1025), dict(points=None), dict(boxes=None))


def caller(f, names, good):
    def call(**kw):
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return f(*args)
    return call


def test_the_entry_points_are_declared_and_loaded(lib):
    from de6d_amd import _lib
    for name in ('det6d_ext_points_in_boxes9', 'det6d_ext_assign_targets9'):
        assert name in _lib.EXT_EXPORTED_SYMBOLS
        assert getattr(lib, name).restype is ctypes.c_int
    assert lib.det6d_ext_version() == b"det6d-hip-ext gfx950 ext3"


def test_points_in_boxes9_bad_arguments_return_minus_one(lib, p):
    names = COMMON + ['box_idx', 'stream']
    call = caller(lib.det6d_ext_points_in_boxes9, names, [64, p, 4, 1, 0, 0, 2, 8, p, 10, None, p, None])
    for bad in BAD_COMMON + (dict(box_idx=None),):
        assert call(**bad) == -1, bad
        assert lib.det6d_ext_last_error().startswith(b"det6d_ext_points_in_boxes9"), bad
    # nothing to do: nothing launched (a launch would fail on a machine without a GPU and could not return 0 there)
    assert call(n_points=0) == 0 and call(m=0) == 0 and call(b=0) == 0
    assert call(n_points=0, points=None) == 0 and call(m=0, boxes=None) == 0


def test_assign_targets9_bad_arguments_return_minus_one(lib, p):
    names = COMMON + ['class_col', 'num_class', 'central_radius', 'box_idx', 'cls_labels', 'box_labels', 'ld_box_labels', 'n_cols',
                      'stream']
    call = caller(lib.det6d_ext_assign_targets9, names, [64, p, 4, 1, 0, 0, 2, 8, p, 10, p, 9, 3, 2.0, p, p, p, 9, 9, None])
    for bad in BAD_COMMON + (dict(class_col=10), dict(num_class=0), dict(central_radius=float('nan')), dict(n_cols=-1),
                             dict(n_cols=11, ld_box_labels=11), dict(ld_box_labels=8), dict(ld_box_labels=1025),
                             dict(box_idx=None, cls_labels=None, box_labels=None)):
        assert call(**bad) == -1, bad
        assert lib.det6d_ext_last_error().startswith(b"det6d_ext_assign_targets9"), bad
    assert call(n_points=0) == 0 and call(m=0) == 0 and call(b=0) == 0
    assert call(n_points=0, box_idx=None, box_labels=None) == 0


def test_the_kernel_holds_no_scratch_and_spills_nothing(ext_path):
    with open(ext_path.replace('.so', '.usage.json')) as fh:
        usage = json.load(fh)['box_targets.hip']
    kernels = {k: u for k, u in usage.items() if 'box_targets9_kernel' in k}
    assert len(kernels) == 1 and len(usage) == 1, sorted(usage)
    for name, u in kernels.items():
        assert not u.get('ScratchSize') and not u.get('VGPRs Spill') and not u.get('SGPRs Spill'), (name, u)
        assert u.get('Dynamic Stack') != 'True', (name, u)
        assert u['VGPRs'] + u.get('AGPRs', 0) <= 64, (name, u)           # 8 waves per SIMD: the box loop hides LDS latency
        assert u['LDS Size'] <= 128 * 64 + 512, (name, u)                # one chunk of 128 box records, two words of control
