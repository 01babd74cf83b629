"""The training-loss entry points of libdet6d_hip_ext.so without a GPU: they are declared and exported, bad arguments return -1
with a message naming the entry point before anything is launched, n = 0 launches nothing, and the kernels hold everything in
registers / LDS."""
import ctypes
import json

import pytest

ENTRIES = ('det6d_ext_head_loss_forward', 'det6d_ext_head_loss_backward', 'det6d_ext_head_loss_workspace_bytes',
           'det6d_ext_centerness_labels', 'det6d_ext_corner_loss')
COMMON = ['n', 'num_class', 'angle_bin_num', 'flags', 'cfg', 'vote_preds', 'vote_reg_labels', 'vote_cls_labels', 'cls_preds',
          'cls_labels', 'reg_preds', 'reg_labels', 'box_labels', 'ld_box_labels']
TENSORS = COMMON[5:13]


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


def cfg_array(**kw):
    values = [1.0, 1.0, 1.0, 0.2, 1.0, 0.2, 1.0, 1.0, 1.0 / 9.0, 0.0, 1.0] + [0.0] * 5
    for k, v in kw.items():
        values[int(k[1:])] = v
    return (ctypes.c_float * 16)(*values)


def caller(f, names, good):
    def call(**kw):
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return f(*args)
    return call


def bad_common():
    return ([dict(n=-1), dict(n=(1 << 24) + 1), dict(num_class=0), dict(num_class=17), dict(angle_bin_num=0),
             dict(angle_bin_num=33), dict(flags=-1), dict(flags=8), dict(cfg=None), dict(ld_box_labels=6),
             dict(ld_box_labels=1025), dict(cfg=cfg_array(c8=-0.5)), dict(cfg=cfg_array(c8=float('nan'))),
             dict(cfg=cfg_array(c0=float('inf'))), dict(cfg=cfg_array(c10=float('nan')))]
            + [{name: None} for name in TENSORS])


def test_the_entry_points_are_declared_and_loaded(lib):
    from de6d_amd import _lib
    from tests.test_ext_boundary import declared
    for name in ENTRIES:
        assert name in _lib.EXT_EXPORTED_SYMBOLS and name in declared()
        assert hasattr(lib, name)
    assert lib.det6d_ext_head_loss_forward.restype is ctypes.c_int and lib.det6d_ext_head_loss_backward.restype is ctypes.c_int
    assert lib.det6d_ext_version() == b"det6d-hip-ext gfx950 ext3"


def test_workspace_bytes(lib):
    ws = lib.det6d_ext_head_loss_workspace_bytes
    assert ws(-1) == -1 and ws((1 << 24) + 1) == -1
    assert ws(0) >= 0 and ws(0) % 16 == 0
    for n in (1, 128, 129, 2048, 20480, 1 << 24):
        assert ws(n) % 16 == 0 and ws(n) >= -(-n // 128) * 32 + 4 * n          # one record per 128 rows and one float per row
    assert ws(20480) <= 2 * (160 * 32 + 4 * 20480)


def test_forward_bad_arguments_return_minus_one(lib, p):
    names = COMMON + ['workspace', 'ws_bytes', 'sums', 'loss_cls', 'loss_box', 'centerness', 'stream']
    ws = lib.det6d_ext_head_loss_workspace_bytes(64)
    call = caller(lib.det6d_ext_head_loss_forward, names, [64, 3, 12, 7, cfg_array()] + [p] * 8 + [9, p, ws, p, p, p, p, None])
    for bad in bad_common() + [dict(ws_bytes=ws - 1), dict(workspace=None), dict(sums=None), dict(ws_bytes=-1)]:
        assert call(**bad) == -1, bad
        assert lib.det6d_ext_last_error().startswith(b"det6d_ext_head_loss_forward"), bad
    # nothing to do: nothing launched (a launch would fail on a machine without a GPU and could not return 0 there)
    assert call(n=0) == 0
    assert call(n=0, vote_preds=None, reg_preds=None, workspace=None, ws_bytes=lib.det6d_ext_head_loss_workspace_bytes(0)) == 0
    assert call(n=0, loss_cls=None, loss_box=None, centerness=None) == 0


def test_backward_bad_arguments_return_minus_one(lib, p):
    names = COMMON + ['sums', 'grad_loss', 'd_vote', 'd_cls', 'd_reg', 'stream']
    call = caller(lib.det6d_ext_head_loss_backward, names, [64, 3, 12, 7, cfg_array()] + [p] * 8 + [9, p, p, p, p, p, None])
    for bad in bad_common() + [dict(sums=None), dict(grad_loss=None), dict(d_vote=None, d_cls=None, d_reg=None)]:
        assert call(**bad) == -1, bad
        assert lib.det6d_ext_last_error().startswith(b"det6d_ext_head_loss_backward"), bad
    assert call(n=0) == 0 and call(n=0, d_vote=None, d_reg=None, sums=None, grad_loss=None) == 0


def test_centerness_and_corner_entries_bad_arguments(lib, p):
    cen = caller(lib.det6d_ext_centerness_labels, ['n', 'points', 'box_labels', 'ld', 'pos_mask', 'out', 'stream'],
                 [64, p, p, 9, p, p, None])
    for bad in (dict(n=-1), dict(n=(1 << 24) + 1), dict(ld=6), dict(ld=1025), dict(points=None), dict(box_labels=None),
                dict(pos_mask=None), dict(out=None)):
        assert cen(**bad) == -1, bad
        assert lib.det6d_ext_last_error().startswith(b"det6d_ext_centerness_labels"), bad
    assert cen(n=0) == 0 and cen(n=0, points=None) == 0
    cor = caller(lib.det6d_ext_corner_loss, ['n', 'pred', 'ld_pred', 'gt', 'ld_gt', 'out', 'stream'], [64, p, 7, p, 7, p, None])
    for bad in (dict(n=-1), dict(n=(1 << 24) + 1), dict(ld_pred=6), dict(ld_gt=6), dict(ld_pred=1025), dict(pred=None),
                dict(gt=None), dict(out=None)):
        assert cor(**bad) == -1, bad
        assert lib.det6d_ext_last_error().startswith(b"det6d_ext_corner_loss"), bad
    assert cor(n=0) == 0 and cor(n=0, pred=None, gt=None) == 0


def test_the_kernels_hold_no_scratch_and_spill_nothing(ext_path):
    with open(ext_path.replace('.so', '.usage.json')) as fh:
        usage = json.load(fh)['head_loss.hip']
    wanted = ('head_loss_forward_kernel', 'head_loss_final_kernel', 'head_loss_pitch_rows_kernel', 'head_loss_backward_kernel',
              'head_centerness_kernel', 'head_corner_loss_kernel')
    assert len(usage) == len(wanted) and all(any(w in k for k in usage) for w in wanted), sorted(usage)
    for name, u in usage.items():
        assert not u.get('ScratchSize') and not u.get('VGPRs Spill') and not u.get('SGPRs Spill'), (name, u)
        assert u.get('Dynamic Stack') != 'True', (name, u)
        assert u['VGPRs'] + u.get('AGPRs', 0) <= 128, (name, u)            # at least 4 waves per SIMD
