"""Host-side mirror of the reference API (no GPU): config, registries, state-dict layout,
BN folding, workload accounting."""
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_config_yaml_and_overrides(tmp_path):
    from de6d_amd.pcdet.config import EasyDict, cfg_from_list, cfg_from_yaml_file, merge_new_config
    cfg = cfg_from_yaml_file(os.path.join(ROOT, 'de6d_amd/cfgs/kitti_models/det6d_car.yaml'), EasyDict())
    assert cfg.MODEL.NAME == 'Det6D' and cfg.MODEL.BACKBONE_3D.SA_CONFIG.NPOINT_LIST[1] == [512, 512]
    assert cfg.DATA_CONFIG.DATA_PROCESSOR[1].NUM_POINTS.test == 16384
    assert cfg.MODEL.POINT_HEAD.get('NOT_THERE', 7) == 7
    cfg_from_list(['MODEL.POST_PROCESSING.SCORE_THRESH', '0.3', 'MODEL.POST_PROCESSING.NMS_CONFIG.NMS_TYPE', 'nms_gpu',
                   'MODEL.POINT_HEAD.SAMPLE_RANGE', '0,128'], cfg)
    assert cfg.MODEL.POST_PROCESSING.SCORE_THRESH == 0.3 and cfg.MODEL.POINT_HEAD.SAMPLE_RANGE == [0, 128]
    with pytest.raises(AssertionError):
        cfg_from_list(['MODEL.NO_SUCH_KEY', '1'], cfg)
    base = tmp_path / 'base.yaml'
    base.write_text("A: {x: 1, y: 2}\nB: 3\n")
    child = tmp_path / 'child.yaml'
    child.write_text("_BASE_CONFIG_: %s\nA: {y: 5}\n" % base)
    merged = cfg_from_yaml_file(str(child), EasyDict())
    assert merged.A.x == 1 and merged.A.y == 5 and merged.B == 3
    assert merge_new_config(EasyDict(), {'K': {'z': [1, {'q': 2}]}}).K.z[1].q == 2


def test_state_dict_layout_equals_the_reference():
    """key names, order and shapes recorded from the reference's own build_network
    (tests/golden/det6d_car_state_dict.json) -> reference checkpoints load unchanged"""
    from de6d_amd.runtime import load_config, build_model
    ref = json.load(open(os.path.join(ROOT, 'tests/golden/det6d_car_state_dict.json')))
    model = build_model(load_config('kitti_models/det6d_car.yaml'))
    sd = model.state_dict()
    assert list(sd.keys()) == ref['keys']
    assert [list(v.shape) for v in sd.values()] == ref['shapes']
    assert sum(p.numel() for p in model.parameters()) == ref['n_params'] == 2356422


def test_registries_and_checkpoint_roundtrip(tmp_path):
    from de6d_amd.pcdet.models import backbones_3d, dense_heads, detectors
    from de6d_amd.runtime import load_config, build_model
    assert 'PointNet2FSMSG' in backbones_3d.__all__ and 'PointHeadBox6DVote' in dense_heads.__all__
    assert 'Det6D' in detectors.__all__
    cfg = load_config('synthetic_models/det6d_tiny.yaml')
    a = build_model(cfg, seed=1)
    path = tmp_path / 'checkpoint_epoch_80.pth'
    torch.save({'epoch': 80, 'it': 1, 'model_state': a.state_dict(), 'version': 'pcdet+0.5.2'}, str(path))

    class Log:
        def info(self, *_):
            pass
    b = build_model(cfg, seed=2)
    b.load_params_from_file(str(path), Log(), to_cpu=True)
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)
    with pytest.raises(NotImplementedError):
        bad = load_config('synthetic_models/det6d_tiny.yaml')
        bad.MODEL['ROI_HEAD'] = {'NAME': 'x'}
        build_model(bad)


def test_bn_folding_matches_torch_eval():
    from de6d_amd.pcdet.ops.pointnet2.pointnet2_batch.pointnet2_modules import fold_sequential
    torch.manual_seed(0)
    seq = torch.nn.Sequential(torch.nn.Conv2d(7, 10, 1, bias=False), torch.nn.BatchNorm2d(10), torch.nn.ReLU(),
                              torch.nn.Conv2d(10, 5, 1, bias=False), torch.nn.BatchNorm2d(5), torch.nn.ReLU())
    for m in seq:
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(); m.running_var.uniform_(0.5, 1.5); m.weight.data.normal_(); m.bias.data.normal_()
    seq.eval()
    x = torch.randn(3, 7, 11, 4)
    want = seq(x).permute(0, 2, 3, 1).reshape(-1, 5).detach().numpy()
    layers = fold_sequential(seq, 8)
    h = np.zeros((3 * 11 * 4, 8), np.float32)
    h[:, :7] = x.permute(0, 2, 3, 1).reshape(-1, 7).numpy()
    for w, s, cout, act in layers:
        h = h @ w
        h[:, :cout] += s
        if act:
            h = np.maximum(h, 0)
    np.testing.assert_allclose(h[:, :5], want, rtol=1e-4, atol=1e-5)
    assert layers[0][0].shape == (8, 12) and layers[1][0].shape == (12, 8)


def test_algorithmic_flops_match_survey():
    from de6d_amd.runtime import load_config, build_model, mlp_flops_per_scene
    model = build_model(load_config('kitti_models/det6d_car.yaml'))
    assert abs(mlp_flops_per_scene(model, 16384) / 1e9 - 22.583) < 0.01


def test_training_mode_is_refused():
    from de6d_amd.runtime import load_config, build_model
    model = build_model(load_config('synthetic_models/det6d_tiny.yaml'))
    model.train()
    with pytest.raises(NotImplementedError):
        model({'batch_size': 1, 'points': torch.zeros((2048, 5))})


def test_any_load_state_dict_drops_the_folded_weights():
    """a plain nn.Module.load_state_dict() must invalidate the folded Conv+BN matrices and bump the version
    captured graphs check"""
    from de6d_amd.runtime import load_config, build_model
    model = build_model(load_config('synthetic_models/det6d_tiny.yaml'), seed=3)
    sa = model.backbone_3d.SA_modules[0]
    sa._folded = {'device': 'stale'}
    model.point_head._folded = {'device': 'stale'}
    v0 = model.weights_version
    model.load_state_dict(model.state_dict())          # NOT the private _load_state_dict
    assert sa._folded is None and model.point_head._folded is None
    assert model.weights_version > v0
    v1 = model.weights_version
    model.eval()                                       # no mode change: nothing to drop
    assert model.weights_version == v1


def test_hoist_plan_is_the_input_only_sampler_chain():
    """runtime.hoist_plan: Det6D's d-fps chain (4096 of the input -> 512 of those -> 256 of those) depends on nothing but
    the input cloud; the s-fps halves (confidence-weighted) do not"""
    from de6d_amd.runtime import load_config, build_model, hoist_plan
    model = build_model(load_config('kitti_models/det6d_car.yaml'), seed=1)
    plan = hoist_plan(list(model.backbone_3d.SA_modules), 16384)
    assert [(s['layer'], s['j'], s['src'], s['lo'], s['hi'], s['m'], s['offset'], s['bias'], s['feeds']) for s in plan] == [
        (0, 0, None, 0, 16384, 4096, 0, 0, True),
        (1, 1, (0, 0), 0, 4096, 512, 512, 0, True),
        (2, 1, (1, 1), 0, 512, 256, 256, 512, False)]


def test_ray_cast_scene_generator():
    """de6d_amd/synthetic.py: beam_scene is deterministic, returns exactly n in-range points through the reference's
    near / far sampling rule, and its density falls with range like a spinning LiDAR's (what makes the ball fill realistic)"""
    from de6d_amd.synthetic import beam_scene, sample_points_rule, points_tensor, beam_batch
    a, b = beam_scene(7, 16384), beam_scene(7, 16384)
    np.testing.assert_array_equal(a, b)
    assert a.shape == (16384, 4) and a.dtype == np.float32 and np.isfinite(a).all()
    assert a[:, 0].min() >= 0 and a[:, 0].max() <= 70.4 and np.abs(a[:, 1]).max() <= 40 and (a[:, 3] >= 0).all() and (a[:, 3] <= 1).all()
    d = np.linalg.norm(a[:, :3], axis=1)
    near, mid = (d < 15).sum(), ((d >= 15) & (d < 30)).sum()
    assert near > 2 * mid > 0                                     # range-dependent density
    assert not np.array_equal(a, beam_scene(8, 16384))
    # the sampling rule: far points (>= 40 m) all survive a down-sampling, short clouds are padded with duplicates
    rng = np.random.default_rng(0)
    pts = np.concatenate([rng.uniform(0, 20, (5000, 4)), np.concatenate([rng.uniform(45, 60, (300, 1)), rng.uniform(-5, 5, (300, 3))], 1)]).astype(np.float32)
    out = sample_points_rule(pts, 2000, np.random.default_rng(1))
    assert out.shape == (2000, 4) and (np.linalg.norm(out[:, :3], axis=1) >= 40).sum() == 300
    short = sample_points_rule(pts[:100], 256, np.random.default_rng(2))
    assert short.shape == (256, 4) and len(np.unique(short, axis=0)) == 100
    flat = points_tensor(beam_batch(3, 2, 2048))
    assert flat.shape == (4096, 5) and (flat[:2048, 0] == 0).all() and (flat[2048:, 0] == 1).all()


def test_scene_pipeline_step_accounting_with_coalesced_passes():
    """ScenePipeline.run counts BATCHES (steps) while its passes hold `merge` batches each: launch order, prefetch distance,
    on_done once per batch in step order with that batch's slice of the pass, and a stream whose length is not a multiple
    of `merge` ends with a full pass that reports its leading batches only.  (Fake groups: the choreography is host logic.)"""
    from de6d_amd.runtime import ScenePipeline

    log = []

    class FakePass(object):
        def __init__(self, name, scenes):
            self.name, self.scenes, self.launched = name, scenes, 0

        def finalize(self):
            return [(self.name, self.launched, i) for i in range(self.scenes)]

    class FakeGroup(object):
        def __init__(self, g, k, scenes):
            self.runners = [FakePass((g, j), scenes) for j in range(k)]
            self.count = k

        def launch_front(self, feed, count):
            self.count = count
            log.append(('front', self.runners[0].name[0], count))

        def launch_rest(self):
            log.append(('rest', self.runners[0].name[0]))
            for r in self.runners[:self.count]:
                r.launched += 1
            return self.runners[:self.count]

    for merge, k, n_groups, prefetch, steps in ((4, 1, 6, 2, 21), (2, 2, 4, 2, 13), (1, 4, 3, 1, 9)):
        pipe = object.__new__(ScenePipeline)
        pipe.merge, pipe.step_scenes, pipe.k, pipe.prefetch, pipe.n_groups = merge, 8, k, prefetch, n_groups
        pipe.groups = [FakeGroup(g, k, 8 * merge) for g in range(n_groups)]
        del log[:]
        seen = []

        def on_done(step, r, preds):
            seen.append((step, r.name, [p[2] for p in preds]))
        assert pipe.run(steps, on_done=on_done) == steps
        assert [s for s, _, _ in seen] == list(range(steps))
        n_pass = -(-steps // merge)
        for step, name, scenes in seen:
            p = step // merge                                   # pass in launch order
            assert name == ((p // k) % n_groups, p % k)
            assert scenes == list(range((step % merge) * 8, (step % merge + 1) * 8))      # that batch's slice of the pass
        fronts = [e for e in log if e[0] == 'front']
        rests = [e for e in log if e[0] == 'rest']
        assert sum(c for _, _, c in fronts) == n_pass and len(rests) == len(fronts)
        # a group's sampler stage is issued `prefetch` groups ahead of its GEMM stage
        first_rest = next(i for i, e in enumerate(log) if e[0] == 'rest')
        assert sum(1 for e in log[:first_rest] if e[0] == 'front') == min(prefetch + 1, len(fronts))

    batches = [torch.full((6, 5), float(i)) for i in range(5)]
    merged = ScenePipeline.coalesce(batches, 2)
    assert len(merged) == 3 and all(m.shape == (12, 5) for m in merged)
    assert merged[2][:6].eq(4).all() and merged[2][6:].eq(0).all()      # cyclic
    assert ScenePipeline.coalesce(batches, 1)[3] is batches[3]


def test_bench_coalesce_factor():
    """bench.py: batches per pass = largest divisor of K that keeps a pass within the target size (80 scenes for 16384-point
    scenes, 32 for larger ones)"""
    import bench
    from bench_legs import scenes_per_pass_target
    assert scenes_per_pass_target(16384) == 80 and scenes_per_pass_target(65536) == 32
    assert bench.coalesce_factor(8, 20, 32) == 4 and bench.coalesce_factor(8, 192, 32) == 4
    assert bench.coalesce_factor(8, 7, 32) == 1 and bench.coalesce_factor(8, 6, 32) == 3
    assert bench.coalesce_factor(4, 20, 32) == 5 and bench.coalesce_factor(4, 192, 32) == 8
    assert bench.coalesce_factor(32, 20, 32) == 1 and bench.coalesce_factor(64, 20, 32) == 1
    assert bench.coalesce_factor(8, 20) == 10 and bench.coalesce_factor(8, 192) == 8 and bench.coalesce_factor(8, 8) == 8
    assert bench.coalesce_factor(4, 20) == 20 and bench.coalesce_factor(8, 7) == 7


def test_timed_span_is_long_enough_for_lock_step_deliveries():
    """bench.py's `value` is K x batch over the MEAN of K-step windows starting on consecutive pass boundaries; that mean
    telescopes to (delivery of the span's last passes - delivery of its first) / passes.  With the passes in flight completing
    in lock-step (16 at the same instant, then nothing for a burst period) a span of few bursts that starts right after a
    burst — as the pre-roll of a whole number of capacities makes it — reads high: rounds 2-4 spanned 768 steps and quoted
    ~5 % too much (profiles/r05_span_bias_r04_vs_r05.txt).  bench_legs.span_windows now spans >= 16 capacities, and the
    least-squares fit printed beside it does not care where the ends fall."""
    from bench_legs import span_windows, window_times, delivery_fit
    merge, in_flight, ahead, K = 10, 16, 4, 20              # 80-scene passes: 16 in the GEMM stage + 4 sampler stages ahead
    capacity, k = (in_flight + ahead) * merge, merge
    period = 5.39e-3                                         # true seconds per pass (14 850 scenes/s at 80 scenes per pass)
    burst = in_flight * period

    def stamps_of(n_steps):                                  # every pass of a burst is delivered when the burst completes
        return {s: (s // merge // in_flight + 1) * burst for s in range(n_steps)}

    def value(n_windows, first):
        stamps = stamps_of(first + n_windows * k + K + capacity)
        w = window_times(stamps, first, k, K, n_windows)
        return K / (sum(w) / len(w)), 1.0 / delivery_fit(stamps, first, first + (n_windows - 1) * k + K)
    true = 1.0 / (period / merge)                            # steps per second
    preroll = 8 * capacity + (-(8 * capacity + 5)) % k       # bench.py: pre-roll of 8 capacities, the windows start on a pass boundary
    first = preroll + 5 - 1                                  # ... after 5 warmup steps
    short, short_fit = value(max(17, -(-768 // k)), first)   # rounds 2-4: 77 windows = 4.8 bursts
    assert short / true > 1.10                               # ... reads > 10 % high on ideal lock-step (measured on the chip: ~5-14 %)
    assert abs(short_fit / true - 1.0) < 0.06                # the fit over the same short span is already within a few per cent
    n = span_windows(capacity, k)
    assert n * k >= 16 * capacity and n >= -(-768 // k)
    long_, long_fit = value(n, first)
    assert abs(long_ / true - 1.0) < 0.045 and abs(long_fit / true - 1.0) < 0.01
    assert span_windows(capacity, k, requested=3) == -(-2 * capacity // k)      # an explicit request: at least two capacities
    assert span_windows(20, 1) == 768                        # one pass per batch: 768 steps are already 38 capacities


def test_mlp_rows_supported_query_mirrors_the_launch_checks():
    """det6d_mlp_rows_supported (host logic of csrc/mlp_rows.hip: chain structure, widths, the 160 KB of LDS a 32-row tile's
    two activation buffers may take) decides fused.mlp_rows_eligible: a stack that does not fit is routed through one
    det6d_linear per layer instead of failing inside the forward pass"""
    import torch
    from de6d_amd.ops import fused
    z = lambda *s: torch.zeros(s)   # noqa: E731
    out = z(4, 1024)
    ok = [[(z(256, 128), 0, None, 256, 128, 1, None, 0), (z(128, 64), 0, None, 128, 64, 1, None, 0), (z(64, 4), 0, None, 64, 1, 0, z(4, 4), 0)]]
    assert fused.mlp_rows_eligible(256, ok)
    towers = [[(z(512, 128), 0, None, 512, 128, 1, None, 0), (z(128, 4), 0, None, 128, 1, 0, z(4, 4), 0)],
              [(z(512, 128), 0, None, 512, 128, 1, None, 0), (z(128, 32), 0, None, 128, 32, 0, z(4, 32), 0)]]
    assert fused.mlp_rows_eligible(512, towers)                       # K-chunked wide input
    assert not fused.mlp_rows_eligible(1024, [[(z(1024, 1024), 0, None, 1024, 1024, 1, None, 0), (z(1024, 1024), 0, None, 1024, 1024, 1, out, 0)]])
    assert not fused.mlp_rows_eligible(96, [[(z(96, 50), 0, None, 96, 50, 1, None, 0), (z(50, 4), 0, None, 50, 1, 0, z(4, 4), 0)]])   # hidden width % 32
    assert not fused.mlp_rows_eligible(256, [[(z(256, 128), 0, None, 256, 128, 1, None, 0)]])    # last layer without an output
    assert not fused.mlp_rows_eligible(256, ok + ok + ok)                                           # three chains

    def stack(k0, *widths):
        ks = (k0,) + widths[:-1]
        last = len(widths) - 1
        return [(z(k, n), 0, None, k, n, int(i < last), z(4, n) if i == last else None, 0) for i, (k, n) in enumerate(zip(ks, widths))]
    # the LDS boundary: 32 x (993 + 257) x 4 = 160 000 bytes fit, 32 x (1025 + 257) x 4 = 164 096 do not
    assert fused.mlp_rows_eligible(992, [stack(992, 256, 32)])
    assert not fused.mlp_rows_eligible(1024, [stack(1024, 256, 32)])
    assert not fused.mlp_rows_eligible(64, [stack(64, 64, 64, 64, 64, 5)])                          # five layers
    assert not fused.mlp_rows_eligible(100, [stack(100, 64, 3)])                                    # k % 32
    assert not fused.mlp_rows_eligible(512, [stack(512, 128, 3), stack(480, 128, 32)])              # two chains, two input widths
    assert not L_supported(fused, [stack(512, 128, 3), stack(480, 128, 32)])
    # every stack tests/test_mlp_rows_gpu.py launches (its group 1) is one the library accepts
    from tests.test_mlp_rows_gpu import STACKS
    for name, chains in STACKS.items():
        assert fused.mlp_rows_eligible(chains[0][0], [stack(k0, *widths) for k0, widths, _ in chains]), name


def L_supported(fused, chains):
    """det6d_mlp_rows_supported itself (mlp_rows_eligible refuses chains of different k0 before it asks the library)"""
    _, counts, arr = fused._rows_descriptors(chains)
    return bool(fused.L.lib().det6d_mlp_rows_supported(len(chains), counts, arr))


# ---- launch plans (include/det6d_ops.h: det6d_*_plan): the host function each fused MLP entry point routes by, asked without a GPU ----
KB160 = 160 * 1024
CHAIN_SETS = {'wide64': (68, 64, 64, 128), 'wide96': (68, 64, 96, 128), 'reg16': (4, 16, 16, 32), 'reg32': (4, 32, 32, 64),
              'lds': (8, 24, 32, 40)}
GROUP_SETS = [(128, 128, 256), (128, 256, 256), (256, 256, 512), (256, 512, 1024)]


def rows_stack(k0, *widths):
    """[(k, n)] of a chain [k0 -> widths...]"""
    return list(zip((k0,) + widths[:-1], widths))


def rows_plan(rows, chains, ldx=None, xcol0=0, aligned=1):
    """det6d_mlp_rows_plan over chains of (k, n) layers (ReLU on hidden layers, only the last one stored, ldw = n, ldo = n; the
    query reads no memory: the pointers only have to be non-NULL) -> (accepted, plan with .name = the route's name)"""
    from de6d_amd import _lib as L
    flat = [(k, n, i == len(c) - 1) for c in chains for i, (k, n) in enumerate(c)]
    arr = (L.RowsLayer * len(flat))()
    for d, (k, n, last) in zip(arr, flat):
        d.w, d.ldw, d.k, d.n, d.act = 0x1000, n, k, n, int(not last)
        if last:
            d.out, d.ldo = 0x1000, n
    counts = (L.c_int * len(chains))(*[len(c) for c in chains])
    plan = L.LaunchPlan()
    rc = L.lib().det6d_mlp_rows_plan(rows, chains[0][0][0] if ldx is None else ldx, xcol0, aligned, len(chains), counts, arr, plan)
    assert rc in (0, -1)
    plan.name = L.ROWS_ROUTES[plan.route] if rc == 0 else None
    if ldx is None:     # over an input as wide as the stack reads no refusal depends on the rows: the _supported query's answer
        assert bool(L.lib().det6d_mlp_rows_supported(len(chains), counts, arr)) == (rc == 0)
    return rc == 0, plan


def chain_plan(lda, c1, c2, c3, ns, b, m, compact=0, capacity=0):
    from de6d_amd import _lib as L
    plan = L.LaunchPlan()
    rc = L.lib().det6d_mlp_chain3_plan(lda, c1, c2, c3, ns, b, m, compact, capacity, plan)
    assert rc in (0, -1)
    plan.name = L.CHAIN_ROUTES[plan.route] if rc == 0 else None
    return rc == 0, plan


def group_plan(c1, c2, c3, ns, b, m, compact=0, capacity=0):
    from de6d_amd import _lib as L
    plan = L.LaunchPlan()
    rc = L.lib().det6d_mlp_group3_plan(c1, c2, c3, ns, b, m, compact, capacity, plan)
    assert rc in (0, -1)
    plan.name = L.GROUP_ROUTES[plan.route] if rc == 0 else None
    return rc == 0, plan


def geometry(plan):
    return (plan.name, plan.tile_rows, plan.grid_x, plan.grid_y, plan.block, plan.lds_bytes)


def test_launch_plans_pin_the_routes_and_their_geometry():
    """Every route of the three fused MLP entry points with the launch geometry the launchers computed inline before the plan
    functions existed; each expectation is a literal with the formula of that code."""
    sa1 = [rows_stack(96, 64, 32, 1)]
    # W: LDS 4 * ((64 + 32) * 32 + 4 * 32 * 97) = 61 952; one wave per 32-row tile, four per workgroup: 16384 / 32 / 4 = 128 (cap 512)
    assert geometry(rows_plan(16384, sa1)[1]) == ('W', 32, 128, 1, 256, 61952)
    # R (rows % 32 != 0): LDS 4 * (2 * 64 * 97 + 64 * 65) = 66 304; 64-row tiles: ceil(16400 / 64) = 257 (cap 512)
    assert geometry(rows_plan(16400, sa1)[1]) == ('R', 64, 257, 1, 256, 66304)
    assert rows_plan(16384, sa1, aligned=0)[1].name == 'G2' and rows_plan(16352, sa1)[1].name == 'G1'   # W, R: 16-byte rows, >= 16384 of them
    # G1, the shape of the launcher bug: 32-row tiles take 4 * 32 * (641 + 65) = 90 368 bytes, 64-row tiles (180 736) do not
    # fit 163 840; one workgroup per CU by LDS: min(16384 / 32, 256 * 1) = 256
    assert geometry(rows_plan(16384, [rows_stack(640, 64, 3)])[1]) == ('G1', 32, 256, 1, 256, 90368)
    # GC: the input in chunks of 256 columns: 4 * 32 * (257 + 129) = 49 408 bytes, 3 per CU; two chains: cap 256 * 3 / 2 = 384
    towers = [rows_stack(512, 128, 1), rows_stack(512, 128, 32)]
    assert geometry(rows_plan(225, towers)[1]) == ('GC', 32, 8, 2, 256, 49408)              # ceil(225 / 32) = 8
    assert geometry(rows_plan(16384, towers)[1]) == ('GC', 32, 384, 2, 256, 49408)          # min(512, 384)
    # G2: 64-row tiles: 4 * 64 * (65 + 65) = 33 280 bytes, 4 per CU: min(16384 / 64, 1024) = 256
    assert geometry(rows_plan(16384, [rows_stack(64, 64, 3)])[1]) == ('G2', 64, 256, 1, 256, 33280)
    assert geometry(rows_plan(16383, [rows_stack(64, 64, 3)])[1]) == ('G1', 32, 512, 1, 256, 16640)   # below 16384 rows: 32-row tiles

    # chain, WIDE: 512 threads take 8 tiles at a time: min(ceil(tiles / 8), 256); LDS 4 * (70 * 64 + 66 * c2 + 128 * c2)
    big = dict(b=8, m=4096)                   # 8 * 4096 * 32 rows = 32 768 tiles: every cap is reached
    for name, lds in (('wide64', 67584), ('wide96', 92416)):
        w = CHAIN_SETS[name]
        assert geometry(chain_plan(*w, 16, 2, 96)[1]) == ('WIDE', 32, 12, 1, 512, lds)       # 2 * 96 * 16 / 32 = 96 tiles -> 12
        assert geometry(chain_plan(*w, 32, 2, 96)[1]) == ('WIDE', 32, 24, 1, 512, lds)       # 192 tiles -> 24
        assert geometry(chain_plan(*w, 32, **big)[1]) == ('WIDE', 32, 256, 1, 512, lds)
        assert geometry(chain_plan(*w, 0, 1, 0, 1, 4096)[1]) == ('WIDE', 32, 16, 1, 512, lds)      # compact: 4096 / 32 / 8 = 16
    # REG: four waves, a tile each: ceil(tiles / 4), dense at most 1024 workgroups, compact lists 2048; no dynamic LDS
    for name in ('reg16', 'reg32'):
        r = CHAIN_SETS[name]
        assert geometry(chain_plan(*r, 16, 2, 96)[1]) == ('REG', 32, 24, 1, 256, 0)          # 96 tiles -> 24
        assert geometry(chain_plan(*r, 32, **big)[1]) == ('REG', 32, 1024, 1, 256, 0)
        assert geometry(chain_plan(*r, 0, 1, 0, 1, 4096)[1]) == ('REG', 32, 32, 1, 256, 0)   # compact: 128 tiles -> 32
        assert geometry(chain_plan(*r, 0, 1, 0, 1, 1 << 20)[1]) == ('REG', 32, 2048, 1, 256, 0)
    # LDS: run-time widths, or centres of two scenes in a tile of the register kernel (ns = 16, odd m): ceil(tiles / 4), at most 1536
    assert geometry(chain_plan(*CHAIN_SETS['lds'], 32, 2, 96)[1]) == ('LDS', 32, 48, 1, 256, 0)     # 192 tiles -> 48
    assert geometry(chain_plan(*CHAIN_SETS['lds'], 32, **big)[1]) == ('LDS', 32, 1536, 1, 256, 0)
    assert geometry(chain_plan(*CHAIN_SETS['reg16'], 16, 2, 3)[1]) == ('LDS', 32, 1, 1, 256, 0)     # 2 * 3 * 16 / 32 = 3 tiles -> 1

    # group, default settings: the head's sets stream, 4 * (32 * (257 + 2 * 129) + 64 + 4 * 64 * 4 + 4 * 256 + 4) = 74 384 bytes: 2
    # per CU; SA3's run the one-pass form on four waves: 4 * (32 * (c1 + 1 + c2 + 1) + 64 + 4 * 64 * 2 + 4) = 35 344 (4 per CU) /
    # 51 728 (3 per CU); a workgroup per 32-row tile, at most 256 x per CU
    want = {(128, 128, 256): ('ONEPASS4', 35344, 1024), (128, 256, 256): ('ONEPASS4', 51728, 768),
            (256, 256, 512): ('STREAM', 74384, 512), (256, 512, 1024): ('STREAM', 74384, 512)}
    for w in GROUP_SETS:
        route, lds, cap = want[w]
        assert geometry(group_plan(*w, 32, 2, 96)[1]) == (route, 32, 192, 1, 256, lds)              # 2 * 96 * 32 / 32 = 192 tiles
        assert geometry(group_plan(*w, 16, 2, 96)[1]) == (route, 32, 96, 1, 256, lds)
        assert geometry(group_plan(*w, 32, **big)[1]) == (route, 32, cap, 1, 256, lds)
        assert geometry(group_plan(*w, 0, 1, 0, 1, 4096)[1]) == (route, 32, 128, 1, 256, lds)       # compact: 4096 / 32
        assert geometry(group_plan(*w, 0, 1, 0, 1, 1 << 20)[1]) == (route, 32, cap, 1, 256, lds)
        assert geometry(group_plan(*w, 16, 0, 0)[1]) == (route, 32, 0, 1, 256, lds)                 # widths only: no grid


def test_launch_plans_hold_their_invariants_over_a_sweep_of_shapes():
    """Accepted plans fit the CU and have a grid; the refusals that used to surface as a failed launch in the middle of a
    forward pass are refusals of the plan; the _supported queries are the plan's answer."""
    import itertools
    from collections import Counter
    from de6d_amd import _lib as L
    seen, refused = Counter(), Counter()

    def check(kind, rows, ok, plan):
        if not ok:
            refused[kind] += 1
            return
        seen[kind, plan.name] += 1
        assert plan.lds_bytes <= KB160 and plan.block in (256, 512) and plan.tile_rows in (32, 64) and plan.grid_y in (1, 2), geometry(plan)
        assert (plan.grid_x >= 1) if rows > 0 else (plan.grid_x == 0), (rows, geometry(plan))

    for depth, k0, last, nchains in itertools.product((1, 2, 3, 4), (32, 96, 256, 512, 640, 992, 1024), (1, 3, 32, 50), (1, 2)):
        for hidden in itertools.product((32, 64, 128, 256), repeat=depth - 1):
            for rows in (0, 1, 225, 16384, 16400):
                ok, plan = rows_plan(rows, [rows_stack(k0, *hidden, last)] * nchains)
                check('rows', rows, ok, plan)
                # two activation buffers of a 32-row tile: the input (or its 256-column chunks) / the widest even-layer input, the widest odd-layer input
                assert ok == (k0 < 1024 or (k0 == 1024 and hidden[:1] in ((32,), (64,), (128,)) or (depth == 1 and last <= 128))), (k0, hidden, last)
    assert not rows_plan(16384, [rows_stack(1024, 256, 32)])[0]
    assert not rows_plan(64, [rows_stack(96, 64, 1)], ldx=100, xcol0=8)[0] and rows_plan(64, [rows_stack(96, 64, 1)], ldx=104, xcol0=8)[0]

    sets = list(CHAIN_SETS.values()) + [(l, c1, c2, c3) for l in (4, 5, 8, 12, 68) for c1, c2, c3 in ((16, 16, 32), (64, 64, 64), (33, 32, 64))]
    for (lda, c1, c2, c3), ns, b, m in itertools.product(sets, (8, 16, 32), (1, 2), (1, 2, 3, 6, 96)):
        ok, plan = chain_plan(lda, c1, c2, c3, ns, b, m)
        check('chain', b * m * ns, ok, plan)
        narrow = lda in (4, 8) and c1 <= 32 and c2 <= 32 and c3 <= 64
        wide = (lda, c1, c3) == (68, 64, 128) and c2 in (64, 96)
        assert ok == (ns in (16, 32) and b * m * ns % 32 == 0 and (narrow or (wide and (ns == 32 or m % 2 == 0)))), (lda, c1, c2, c3, ns, b, m)
        if ok and not wide:
            reg = lda == 4 and (c1, c2, c3) in ((16, 16, 32), (32, 32, 64)) and (ns == 32 or m % 2 == 0)
            assert plan.name == ('REG' if reg else 'LDS')
        okc, planc = chain_plan(lda, c1, c2, c3, ns, 1, m, 1, 128 * m)          # the compact entry: register kernels only
        check('chain', 128 * m, okc, planc)
        assert okc == (wide or (lda == 4 and (c1, c2, c3) in ((16, 16, 32), (32, 32, 64)))) and (not okc or planc.name in ('WIDE', 'REG'))
        assert chain_plan(lda, c1, c2, c3, ns, 0, 0)[0] == (ns in (16, 32) and (narrow or wide))      # the widths alone
        assert not chain_plan(lda, c1, c2, c3, ns, 1, m, 1, 128 * m + 32)[0]
    # the refusals by name: a wide chain / any chain whose tiles would pair centres of two scenes or split a tile
    for w in ('wide64', 'wide96'):
        assert not chain_plan(*CHAIN_SETS[w], 16, 1, 3)[0] and not chain_plan(*CHAIN_SETS[w], 16, 2, 3)[0] and chain_plan(*CHAIN_SETS[w], 16, 1, 6)[0]
    assert not chain_plan(*CHAIN_SETS['reg16'], 16, 1, 3)[0] and not chain_plan(5, 16, 16, 32, 32, 1, 2)[0]

    for (c1, c2, c3), ns, b, m, compact in itertools.product(GROUP_SETS + [(128, 128, 128), (256, 512, 512)], (8, 16, 32), (1, 2), (1, 2, 3), (0, 1)):
        ok, plan = group_plan(c1, c2, c3, ns, b, m, compact, 128 * m)
        check('group', 128 * m if compact else b * m * ns, ok, plan)
        assert ok == ((c1, c2, c3) in GROUP_SETS and (compact == 1 or (ns in (16, 32) and (ns == 32 or m % 2 == 0)))), (c1, c2, c3, ns, b, m, compact)
        widths_only = (c1, c2, c3) in GROUP_SETS and (compact == 1 or ns in (16, 32))
        assert group_plan(c1, c2, c3, ns, 0, 0, compact)[0] == widths_only == bool(L.lib().det6d_mlp_group3_supported(c1, c2, c3, ns, compact))
    assert not group_plan(128, 128, 256, 16, 2, 3)[0] and not group_plan(128, 128, 256, 0, 1, 0, 1, 96)[0]

    # not vacuous: every route the shipped settings can take was accepted somewhere, every entry point refused something
    for key in [('rows', r) for r in L.ROWS_ROUTES] + [('chain', r) for r in L.CHAIN_ROUTES] + [('group', 'STREAM'), ('group', 'ONEPASS4')]:
        assert seen[key] >= 1, (key, seen)
    assert all(refused[k] >= 1 for k in ('rows', 'chain', 'group')), refused


def test_route_switches_are_read_by_the_plan_functions():
    """the experiments build's route switches reach the launch through the plan: eight waves per tile for the head's groups once
    their streaming form is off, no wide chain kernel on either entry with DET6D_CHAIN_NO_WIDE (switches are read once per
    process: a child)"""
    import subprocess
    import sys
    from de6d_amd import _build
    _build.build(experiments=True)
    code = ("from tests.test_host_logic import chain_plan, group_plan, geometry, CHAIN_SETS\n"
            "w = CHAIN_SETS['wide64']\n"
            "print(geometry(group_plan(256, 512, 1024, 32, 2, 96)[1]), geometry(group_plan(128, 256, 256, 32, 2, 96)[1]),"
            " chain_plan(*w, 32, 2, 96)[0], chain_plan(*w, 0, 1, 0, 1, 4096)[0], chain_plan(*CHAIN_SETS['reg16'], 32, 2, 96)[1].name)")
    env = dict(os.environ, DET6D_EXPERIMENTS_LIB='1', DET6D_GROUP_STREAM='0', DET6D_CHAIN_NO_WIDE='1', DET6D_CHAIN_LDS='1')
    out = subprocess.run([sys.executable, '-c', code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    # one-pass, eight waves: 4 * (32 * (257 + 513) + 64 + 8 * 64 * 4 + 4) = 107 024 bytes, one workgroup per CU; SA3 stays at four
    assert out.stdout.strip() == "('ONEPASS8', 32, 192, 1, 512, 107024) ('ONEPASS4', 32, 192, 1, 256, 51728) False False LDS", out.stdout


def test_fused_predicates_ask_the_plan():
    """fused.chain_eligible / group_kernel_eligible at a (b, m): what the library would refuse is not offered to it"""
    from de6d_amd.ops import fused
    layers = lambda *c: [(None, None, n, 1) for n in c]   # noqa: E731
    wide, narrow = layers(64, 64, 128), layers(16, 16, 32)
    assert not fused.chain_eligible(68, wide, 16, b=1, m=3) and not fused.chain_eligible(4, narrow, 16, b=1, m=3)
    assert fused.chain_eligible(68, wide, 16, b=1, m=6) and fused.chain_eligible(4, narrow, 16, b=1, m=6)
    assert fused.chain_eligible(68, wide, 16) and fused.chain_eligible(68, layers(64, 96, 128), 32) and fused.chain_eligible(8, layers(24, 32, 40), 32)
    assert not fused.chain_eligible(8, narrow, 8) and not fused.chain_eligible(12, narrow, 16) and not fused.chain_eligible(5, narrow, 16)
    assert not fused.chain_eligible(4, narrow[:2], 16) and not fused.chain_eligible(4, [(None, None, 16, 0)] + narrow[1:], 16)
    assert fused.chain_compact_eligible(68, wide) and fused.chain_compact_eligible(4, narrow) and not fused.chain_compact_eligible(8, narrow)
    group = layers(128, 128, 256)
    assert fused.group_kernel_eligible(group, 16, False) and fused.group_kernel_eligible(group, 16, False, b=1, m=2)
    assert not fused.group_kernel_eligible(group, 16, False, b=1, m=3) and fused.group_kernel_eligible(group, 16, True, b=1, m=3)
    assert not fused.group_kernel_eligible(layers(128, 128, 128), 16, False) and not fused.group_kernel_eligible(group, 8, False)


def test_group_route_names_one_of_six_routes():
    """pointnet2_modules.group_route at the shapes of the configs: kitti det6d_car's SA1 (point rows of 4 floats), SA2 (68),
    SA3 (132) and head (260), det6d_tiny's SA1 (4) and SA2 (20); and the refusals of tests/gpu_scripts/sa_odd_centres.py: a
    wide chain on dense rows, chained by its widths, refused at three centres, taken at four"""
    from de6d_amd.pcdet.ops.pointnet2.pointnet2_batch.pointnet2_modules import group_route
    layers = lambda *c: [(None, None, n, 1) for n in c]   # noqa: E731
    # (lda, layers, nsample, compact rows, in the expand set, b, m)
    assert group_route(4, layers(16, 16, 32), 16, True, False, 2, 4096) == 'compact_chain'
    assert group_route(4, layers(32, 32, 64), 32, True, False, 2, 4096) == 'compact_chain'
    assert group_route(68, layers(64, 96, 128), 32, True, False, 2, 1024) == 'compact_chain'
    assert group_route(132, layers(128, 128, 256), 16, True, True, 2, 512) == 'compact_group'
    assert group_route(260, layers(256, 512, 1024), 32, True, True, 2, 256) == 'compact_group'
    assert group_route(132, layers(128, 128, 256), 16, True, False, 2, 512) == 'compact_layers'     # no partial sums: no group kernel
    assert group_route(4, layers(8, 8, 16), 16, True, False, 3, 512) == 'compact_layers'            # widths without a register chain
    assert group_route(20, layers(16, 16, 32), 16, True, True, 3, 256) == 'compact_layers'
    assert group_route(4, layers(8), 4, True, False, 2, 64) == 'compact_layers'                     # a single layer
    assert group_route(4, layers(16, 16, 32), 16, False, False, 2, 4096) == 'dense_chain'
    assert group_route(4, layers(8, 8, 16), 32, False, False, 3, 512) == 'dense_chain'              # the LDS chain takes any narrow widths
    assert group_route(68, layers(64, 64, 128), 16, False, False, 2, 1024) == 'dense_chain'
    assert group_route(132, layers(128, 256, 256), 32, False, True, 2, 512) == 'dense_group'
    assert group_route(260, layers(256, 256, 512), 16, False, True, 2, 256) == 'dense_group'
    assert group_route(132, layers(128, 256, 256), 32, False, False, 2, 512) == 'dense_layers'
    assert group_route(20, layers(16, 16, 32), 16, False, True, 3, 256) == 'dense_layers'
    assert group_route(8, layers(16, 16, 32), 12, False, True, 2, 63) == 'dense_layers'             # nsample off the tiles
    assert group_route(260, layers(256, 256, 512), 16, False, True, 1, 3) == 'dense_layers'         # odd m with nsample 16
    for wide in (layers(64, 64, 128), layers(64, 96, 128)):
        assert group_route(68, wide, 16, False, False) == 'dense_chain'                             # _prepare's question: b = m = 0
        assert group_route(68, wide, 16, False, False, 1, 3) == 'dense_layers'
        assert group_route(68, wide, 16, False, False, 1, 4) == 'dense_chain'


def test_bench_refuses_more_ranks_than_devices():
    """`bench.py --gpus N` with fewer than N visible devices exits non-zero BEFORE any rank is started or any rendezvous is
    attempted (a rank that left alone would keep the others waiting for the store's ten-minute time-out); decided from
    torch.cuda.device_count(), which does not initialise the GPU.  Here: no device at all."""
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("needs a machine with fewer than two devices")
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'DET6D_BENCH_BACKEND')}
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '4', '--warmup', '1'], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode != 0
    assert 'visible device' in (out.stderr + out.stdout)


def test_hardware_queue_rule(monkeypatch):
    """GPU_MAX_HW_QUEUES is read when HIP initialises: importing the package exports 24 while nothing has touched the GPU;
    require_hw_queues raises (instead of the round-4 warning) when fewer queues than streams are in effect, unless the caller
    asks for the aliased form"""
    import subprocess
    import sys
    import de6d_amd
    from de6d_amd import runtime
    # a fresh interpreter that has not chosen a value gets 24 from the import, one that has keeps its own
    code = "import os; os.environ.pop('GPU_MAX_HW_QUEUES', None); import de6d_amd; print(os.environ['GPU_MAX_HW_QUEUES'], de6d_amd.HW_QUEUES_AT_IMPORT)"
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.stdout.split() == ['24', 'None'], out.stdout + out.stderr
    code = "import os; os.environ['GPU_MAX_HW_QUEUES'] = '8'; import de6d_amd; print(os.environ['GPU_MAX_HW_QUEUES'])"
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.stdout.split() == ['8']
    monkeypatch.setattr(de6d_amd, 'HW_QUEUES_AT_IMPORT', None)
    monkeypatch.setenv('GPU_MAX_HW_QUEUES', '24')
    assert runtime.require_hw_queues(22) == 24
    monkeypatch.setenv('GPU_MAX_HW_QUEUES', '4')
    with pytest.raises(RuntimeError, match='GPU_MAX_HW_QUEUES'):
        runtime.require_hw_queues(22)
    assert runtime.require_hw_queues(22, allow_aliasing=True) == 4
    # HIP initialised before the import with the default queues (the ROS-node shape): the value of THAT moment counts
    monkeypatch.setattr(de6d_amd, 'HW_QUEUES_AT_IMPORT', 4)
    monkeypatch.setenv('GPU_MAX_HW_QUEUES', '24')
    with pytest.raises(RuntimeError):
        runtime.require_hw_queues(6)


def test_whole_path_scalars_put_the_driver_timed_fraction_at_the_top_of_roofline():
    """round-5 review item 6: roofline.frac is the DRIVER-TIMED whole-path fraction (algorithmic GFLOP per scene x value /
    peak); the launch-by-launch family figures and the dominant launch become top-level scalars beside it; with clock
    samples the fraction at the held clock is stated next to the nominal one"""
    from bench_legs import whole_path_scalars, MFMA_F32_PEAK_TFLOPS
    roof = {"frac": 0.659, "achieved": 103.7, "algorithmic_gflop_per_pass": 519.11, "saturated": {"frac": 0.736},
            "dominant_launch": {"frac": 0.764}}
    out = whole_path_scalars(roof, 80, 15009.82, {"sclk_mhz": 2200.0, "power_w": 1000.0})
    assert out["family_frac_idle"] == 0.659 and out["family_frac_saturated"] == 0.736 and out["dominant_launch_frac"] == 0.764
    assert abs(out["algorithmic_gflop_per_scene"] - 6.4889) < 1e-3
    assert abs(out["achieved"] - 6.488875 * 15009.82 / 1e3) < 0.01
    assert out["frac"] == out["whole_path_frac"] == round(out["achieved"] / MFMA_F32_PEAK_TFLOPS, 4) or abs(out["frac"] - 0.6192) < 2e-4
    assert out["sclk_mhz"] == 2200.0 and out["power_w"] == 1000.0
    assert abs(out["whole_path_frac_at_held_clock"] - out["frac"] * 2400.0 / 2200.0) < 1e-4
    assert all(not isinstance(out[k], dict) for k in ("whole_path_frac", "family_frac_idle", "family_frac_saturated", "dominant_launch_frac"))
