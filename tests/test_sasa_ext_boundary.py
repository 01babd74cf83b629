"""The SASA entry points of libdet6d_hip_ext.so without a GPU: they are declared and exported, bad arguments return -1 with a
message naming the entry point before anything is launched, no rows launch nothing, and the kernels hold everything in
registers / LDS."""
import ctypes
import json

import pytest

ENTRIES = ('det6d_ext_points_in_boxes7', 'det6d_ext_sasa_forward', 'det6d_ext_sasa_backward', 'det6d_ext_sasa_workspace_bytes')
COMMON = ['n_segments', 'segments', 'b', 'm', 'boxes', 'ld_boxes', 'extra_width', 'flags', 'func', 'alpha', 'gamma']


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


def segments(p, n=3, **kw):
    """n good segments of 100 points per scene; kw: field=(index, value) overrides"""
    from de6d_amd import _lib
    segs = (_lib.SasaSegment * max(n, 1))()
    for i in range(n):
        segs[i].coords, segs[i].m, segs[i].ld, segs[i].xyz_col, segs[i].weight = p.value, 100, 4, 1, 0.5
        segs[i].scores, segs[i].labels, segs[i].d_scores = p.value, p.value, p.value
    for field, (i, value) in kw.items():
        setattr(segs[i], field, value)
    return segs


def caller(f, names, good):
    def call(**kw):
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return f(*args)
    return call


def bad_common(p):
    nan = float('nan')
    return [dict(n_segments=-1), dict(n_segments=9, segments=segments(p, 9)), dict(segments=None), dict(b=-1), dict(b=4097),
            dict(m=-1), dict(m=1025), dict(ld_boxes=6), dict(ld_boxes=1025), dict(flags=-1), dict(flags=4), dict(func=2),
            dict(func=-1), dict(flags=1, extra_width=None), dict(alpha=nan), dict(gamma=nan), dict(gamma=-1.0),
            dict(gamma=float('inf')), dict(boxes=None),
            dict(segments=segments(p, m=(1, -1))), dict(segments=segments(p, ld=(0, 2))), dict(segments=segments(p, ld=(2, 1025))),
            dict(segments=segments(p, xyz_col=(1, 2))), dict(segments=segments(p, xyz_col=(1, -1))),
            dict(segments=segments(p, weight=(0, nan))), dict(segments=segments(p, weight=(2, float('inf')))),
            dict(segments=segments(p, m=(0, 1 << 23)), b=3)]


def test_the_entry_points_are_declared_and_loaded(lib):
    from de6d_amd import _lib
    from tests.test_ext_boundary import declared
    for name in ENTRIES:
        assert name in _lib.EXT_EXPORTED_SYMBOLS and name in declared()
        assert hasattr(lib, name)
    assert lib.det6d_ext_sasa_forward.restype is ctypes.c_int and lib.det6d_ext_sasa_backward.restype is ctypes.c_int
    assert lib.det6d_ext_version() == b"det6d-hip-ext gfx950 ext3"
    assert ctypes.sizeof(_lib.SasaSegment) == 48              # the layout of det6d_ext_sasa_segment on LP64


def test_workspace_bytes(lib, p):
    ws = lib.det6d_ext_sasa_workspace_bytes
    assert ws(-1, segments(p), 2) == -1 and ws(9, segments(p, 9), 2) == -1 and ws(3, None, 2) == -1 and ws(3, segments(p), 4097) == -1
    assert ws(3, segments(p, m=(0, 1 << 23)), 3) == -1
    assert ws(0, None, 2) == 0 and ws(3, segments(p), 0) == 0
    assert ws(3, segments(p), 8) == 3 * 4 * 16                 # 800 rows: four slabs of 256 per segment, 16 bytes per record
    assert ws(3, segments(p, weight=(1, 0.0)), 8) == 2 * 4 * 16 and ws(3, segments(p, scores=(1, None)), 8) == 2 * 4 * 16


def test_points_in_boxes7_bad_arguments_return_minus_one(lib, p):
    names = ['n_points', 'points', 'ld_points', 'xyz_col', 'bs_col', 'n_per_scene', 'b', 'm', 'boxes', 'ld_boxes', 'extra_width',
             'box_idx', 'stream']
    call = caller(lib.det6d_ext_points_in_boxes7, names, [64, p, 4, 1, 0, 1, 2, 8, p, 7, None, p, None])
    for bad in (dict(n_points=-1), dict(n_points=(1 << 24) + 1), dict(b=-1), dict(b=4097), dict(m=-1), dict(m=1025), dict(ld_boxes=6),
                dict(ld_boxes=1025), dict(ld_points=2), dict(ld_points=1025), dict(xyz_col=2), dict(xyz_col=-1), dict(bs_col=4),
                dict(bs_col=-1, n_per_scene=0), dict(box_idx=None), dict(points=None), dict(boxes=None)):
        assert call(**bad) == -1, bad
        assert lib.det6d_ext_last_error().startswith(b"det6d_ext_points_in_boxes7"), bad
    # nothing to do: nothing launched (a launch would fail on a machine without a GPU and could not return 0 there)
    assert call(n_points=0) == 0 and call(b=0) == 0 and call(m=0) == 0 and call(n_points=0, points=None, boxes=None) == 0
    assert call(m=0, ld_boxes=10, extra_width=p) == 0


def test_forward_bad_arguments_return_minus_one(lib, p):
    names = COMMON + ['workspace', 'ws_bytes', 'sums', 'stream']
    ws = lib.det6d_ext_sasa_workspace_bytes(3, segments(p), 2)
    call = caller(lib.det6d_ext_sasa_forward, names, [3, segments(p), 2, 8, p, 10, p, 1, 0, 0.25, 2.0, p, ws, p, None])
    for bad in bad_common(p) + [dict(ws_bytes=ws - 1), dict(ws_bytes=-1), dict(workspace=None), dict(sums=None),
                                dict(segments=segments(p, coords=(1, None))), dict(flags=2, segments=segments(p, labels=(2, None)))]:
        assert call(**bad) == -1, bad
        assert lib.det6d_ext_last_error().startswith(b"det6d_ext_sasa_forward"), bad
    # no rows: nothing launched
    assert call(n_segments=0) == 0 and call(n_segments=0, segments=None, workspace=None, ws_bytes=0) == 0
    assert call(b=0, boxes=None, workspace=None, ws_bytes=0, sums=None) == 0
    skipped = segments(p, scores=(0, None), weight=(1, 0.0), m=(2, 0))
    assert call(segments=skipped, workspace=None, ws_bytes=0) == 0


def test_backward_bad_arguments_return_minus_one(lib, p):
    names = COMMON + ['sums', 'grad_loss', 'grad_stride', 'stream']
    call = caller(lib.det6d_ext_sasa_backward, names, [3, segments(p), 2, 8, p, 10, p, 1, 0, 0.25, 2.0, p, p, 0, None])
    no_labels = segments(p, labels=(1, None))
    for bad in [b for b in bad_common(p) if b != dict(boxes=None)] + [
            dict(sums=None), dict(grad_loss=None), dict(grad_stride=-1), dict(grad_stride=5),
            dict(segments=segments(p, d_scores=(2, None))), dict(segments=no_labels, boxes=None),
            dict(segments=segments(p, labels=(1, None), coords=(1, None)))]:
        assert call(**bad) == -1, bad
        assert lib.det6d_ext_last_error().startswith(b"det6d_ext_sasa_backward"), bad
    assert call(n_segments=0) == 0 and call(b=0, sums=None, grad_loss=None) == 0
    assert call(segments=segments(p, scores=(0, None), weight=(1, 0.0), m=(2, 0)), sums=None) == 0


def test_the_kernels_hold_no_scratch_and_spill_nothing(ext_path):
    with open(ext_path.replace('.so', '.usage.json')) as fh:
        usage = json.load(fh)['sasa_loss.hip']
    wanted = ('points_in_boxes7_kernel', 'sasa_forward_kernel', 'sasa_final_kernel', 'sasa_backward_kernel')
    assert len(usage) == len(wanted) and all(any(w in k for k in usage) for w in wanted), sorted(usage)
    for name, u in usage.items():
        assert not u.get('ScratchSize') and not u.get('VGPRs Spill') and not u.get('SGPRs Spill'), (name, u)
        assert u.get('Dynamic Stack') != 'True', (name, u)
        assert u['VGPRs'] + u.get('AGPRs', 0) <= 128, (name, u)            # at least 4 waves per SIMD
        assert u['LDS Size'] <= 8 * 1024, (name, u)                          # a chunk of 128 box records and the reduction
