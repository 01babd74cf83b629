"""Launch traces: which entry points of the two libraries a pass calls, with which arguments, in which order.

Every route of a radius group gives the same bits, so the bit-exact GPU suite cannot see a change that sends a group down another
route; the traces under tests/traces/ pin the routes (tests/test_launch_trace.py).  `record()` replaces four functions of
de6d_amd._lib: call / call_ext append an entry and return 0, require_cuda becomes a no-op, stream_ptr returns None.  With these
stubs a model runs on CPU tensors with the library built and no GPU; the det6d_*_plan, _supported, _capacity and
_workspace_bytes queries still go to the real library, so the routes are the real ones.  `record(passthrough=True)` only listens:
the real call runs (tests/test_model_gpu.py compares such a recording with the CPU one).

An entry is [name, argument, ...]: ints and floats as they are, a pointer as "p" or null, a ctypes.byref as its pointee, a
structure as a dict of its fields, a ctypes array as a list.  Pointer identity is not recorded: allocator reuse would make it
depend on the lifetimes of temporaries, and a wrong buffer is what the bit-exact suite catches.

`python -m tests.launch_trace CASE` prints the trace of one case as JSON (the switches that are read at import need a process of
their own: CASES names their environment); `--write` stores every case under tests/traces/ — done once, on the commit before the
SA-layer refactor, and not since."""
import contextlib
import ctypes
import json
import numbers
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE_DIR = os.path.join(ROOT, 'tests', 'traces')


def encode(v):
    if v is None or isinstance(v, str):
        return v
    if isinstance(v, ctypes.c_void_p):
        return 'p' if v.value else None
    if isinstance(v, ctypes.Structure):
        out = {}
        for name, kind in v._fields_:
            field = getattr(v, name)
            out[name] = ('p' if field else None) if kind is ctypes.c_void_p else encode(field)
        return out
    if isinstance(v, ctypes.Array):
        return [encode(e) for e in v]
    if hasattr(v, '_obj'):                       # ctypes.byref(x)
        return encode(v._obj)
    if hasattr(v, 'value'):                      # c_int, c_uint64, ...
        return encode(v.value)
    if isinstance(v, numbers.Integral):
        return int(v)
    if isinstance(v, numbers.Real):
        return float(v)
    raise TypeError("launch trace: cannot encode %r" % (v,))


@contextlib.contextmanager
def record(passthrough=False):
    """-> the list the entries are appended to while the block runs"""
    from de6d_amd import _lib as L
    trace = []
    saved = {name: getattr(L, name) for name in ('call', 'call_ext', 'require_cuda', 'stream_ptr')}

    def listener(real):
        def call(name, *args):
            trace.append([name] + [encode(a) for a in args])
            return real(name, *args) if passthrough else 0
        return call
    L.call, L.call_ext = listener(saved['call']), listener(saved['call_ext'])
    if not passthrough:
        L.require_cuda = lambda *tensors: None
        L.stream_ptr = lambda device=None: None
    try:
        yield trace
    finally:
        for name, fn in saved.items():
            setattr(L, name, fn)


# ---- the cases ----------------------------------------------------------------------------------------------------------
def run_modules(model, b, n, points=None):
    """backbone + head of one pass (no post-processing) -> batch_dict"""
    bd = {'batch_size': b, 'points': torch.zeros((b * n, 5)) if points is None else points}
    with torch.no_grad():
        for module in model.module_list:
            bd = module(bd)
    return bd


def model_case(cfg, b, n):
    def run():
        from de6d_amd.runtime import load_config, build_model
        model = build_model(load_config(cfg))
        with record() as trace:
            run_modules(model, b, n)
        return trace
    return run


def loss_case(**kw):
    """a pass of det6d_tiny_loss.yaml, then one training step: loss and backward"""
    def run():
        from de6d_amd.runtime import load_config, build_model
        b, n = 2, 2048
        model = build_model(load_config('synthetic_models/det6d_tiny_loss.yaml'))
        gt = torch.zeros((b, 4, 10))
        gt[:, :, 3:6] = 1.0
        gt[:, :, 9] = 1.0
        with record() as trace:
            bd = run_modules(model, b, n)
            bd['gt_boxes'] = gt
            loss = model.get_training_loss(bd, requires_grad=True, **kw)[0]
            loss.backward()
        return trace
    return run


def layer_case(b, n, c, centres, supplied=False, **kw):
    """one set-abstraction layer through forward()"""
    def run():
        from de6d_amd.pcdet.ops.pointnet2.pointnet2_batch import pointnet2_modules as modules
        torch.manual_seed(0)
        sa = modules.PointnetSAModuleFSMSG(npoint_list=[centres], sample_range_list=[[0, -1]], sample_method_list=['d-fps'],
                                           **kw).eval()
        xyz = torch.zeros((b, n, 3))
        feats = torch.zeros((b, c, n)) if c else None
        with record() as trace, torch.no_grad():
            sa(xyz, feats, new_xyz=torch.zeros((b, centres, 3)) if supplied else None)
        return trace
    return run


EXPERIMENTS = {'DET6D_EXPERIMENTS_LIB': '1'}
DENSE = {'DET6D_DENSE_ROWS': '1'}
NARROW = [4, 16, 16, 32]

#: name -> (function returning the trace, environment of the child process it needs or None)
CASES = {
    'tiny_b3_n2048': (model_case('synthetic_models/det6d_tiny.yaml', 3, 2048), None),
    'tiny_b1_n777': (model_case('synthetic_models/det6d_tiny.yaml', 1, 777), None),
    'car_b2_n16384': (model_case('kitti_models/det6d_car.yaml', 2, 16384), None),
    '3class_b1_n16384': (model_case('kitti_models/det6d_3class.yaml', 1, 16384), None),
    'sloped_car_b1_n16384': (model_case('slopedkitti_models/det6d_car.yaml', 1, 16384), None),
    'tiny_ffps_b2_n2048': (model_case('synthetic_models/det6d_tiny_ffps.yaml', 2, 2048), None),
    'tiny_cfps_b2_n2048': (model_case('synthetic_models/det6d_tiny_cfps.yaml', 2, 2048), None),
    'tiny_dffps_b2_n2048': (model_case('synthetic_models/det6d_tiny_dffps.yaml', 2, 2048), None),
    'tiny_loss_towers': (loss_case(towers=True), None),
    'tiny_loss_head': (loss_case(head=True), None),
    'tiny_b3_n2048_dense_rows': (model_case('synthetic_models/det6d_tiny.yaml', 3, 2048), DENSE),
    'car_b1_n16384_dense_rows': (model_case('kitti_models/det6d_car.yaml', 1, 16384), DENSE),     # the dense group kernel
    'car_b1_n16384_no_expand': (model_case('kitti_models/det6d_car.yaml', 1, 16384), dict(EXPERIMENTS, DET6D_NO_EXPAND='1')),
    'car_b1_n16384_no_group_kernel': (model_case('kitti_models/det6d_car.yaml', 1, 16384),
                                      dict(EXPERIMENTS, DET6D_NO_GROUP_KERNEL='1')),
    'car_b1_n16384_compact_no_chain': (model_case('kitti_models/det6d_car.yaml', 1, 16384),
                                       dict(EXPERIMENTS, DET6D_COMPACT_NO_CHAIN='1')),
    'car_b1_n16384_compact_split0': (model_case('kitti_models/det6d_car.yaml', 1, 16384),
                                     dict(EXPERIMENTS, DET6D_COMPACT_SPLIT='0')),
    'layer_one_group': (layer_case(2, 512, 0, 64, radii=[1.0], nsamples=[4], mlps=[[0, 8]]), None),
    'layer_dilated_three_groups': (layer_case(2, 512, 4, 64, radii=[0.5, 1.0, 2.0], nsamples=[8, 16, 6], mlps=[NARROW] * 3,
                                              dilated_radius_group=True, aggregation_mlp=[64], confidence_mlp=[32]), None),
    'layer_two_groups_63': (layer_case(2, 512, 4, 63, radii=[0.5, 1.0], nsamples=[12, 48], mlps=[NARROW, [4, 32, 32, 64]],
                                       aggregation_mlp=[64]), None),
    # the layer of tests/gpu_scripts/sa_odd_centres.py: dense wide chains that the library refuses at three centres
    'layer_odd_centres_dense_rows': (layer_case(1, 64, 64, 3, supplied=True, radii=[0.8, 1.6], nsamples=[16, 16],
                                                mlps=[[64, 64, 64, 128], [64, 64, 96, 128]]), DENSE),
}


def trace_of(name):
    """the trace of a case as JSON data; in a child process where the case needs an environment of its own"""
    run, env = CASES[name]
    if env is None or all(os.environ.get(k) == v for k, v in env.items()):
        return json.loads(json.dumps(run()))
    out = subprocess.run([sys.executable, '-m', 'tests.launch_trace', name], env=dict(os.environ, **env), cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    return json.loads(out.stdout)


def fixture(name):
    with open(os.path.join(TRACE_DIR, name + '.json')) as fh:
        return json.load(fh)


if __name__ == '__main__':
    if sys.argv[1] == '--write':
        os.makedirs(TRACE_DIR, exist_ok=True)
        for case in CASES:
            with open(os.path.join(TRACE_DIR, case + '.json'), 'w') as fh:
                fh.write('[\n' + ',\n'.join(json.dumps(e) for e in trace_of(case)) + '\n]\n')
    else:
        print(json.dumps(CASES[sys.argv[1]][0]()))
