"""Plain-layer stacks in one launch (csrc/mlp_rows.hip, det6d_mlp_rows) over every route its launcher accepts.

The launcher takes run-time widths and picks one of five device routes (ids below carry the intended one):
  G1  mlp_rows_kernel<false,1>   general stacks, 32-row tiles
  G2  mlp_rows_kernel<false,2>   every layer at most two column tiles, >= 16384 rows: 64-row tiles
  GC  mlp_rows_kernel<true,1>    k0 >= 512, k0 % 256 == 0, every first layer <= 128 wide: the input in K-chunks of 256
  W   mlp_rows_wave_kernel       [96 -> 64 -> 32 -> n <= 32], >= 16384 rows, rows % 32 == 0, 16-byte rows
  R   mlp_rows_resident_kernel   the same stack when rows % 32 != 0

Two references, both independent of the kernel:
  exact   inputs, weights and shifts are small integers times a power of two, chosen so that every partial sum of every layer is
          an integer multiple of the layer's grid G_l below 2^24 G_l (asserted per layer on the float64 reference: a condition on
          the INPUTS, not a tolerance).  Then every fp32 summation order is exact, the float64 result cast to fp32 is the only
          right answer, and the comparison is assert_array_equal.  NumPy only: these cases carry the large row counts.
  oracle  normal floats against oracle_ops.linear layer by layer, bit for bit: the kernel's stated contract (the ascending-k
          fma chain of det6d_linear).

Every output buffer is wider (and by three rows longer) than what the layer writes and pre-filled with a sentinel; the whole
buffer is compared, so a write outside [ocol0, ocol0 + n) x [0, rows) fails.  Input columns outside [xcol0, xcol0 + k0), weight
rows outside [wrow0, wrow0 + k) and weight columns [n, ldw) are NaN: include/det6d_ops.h asks for no zero padding (a layer is
W[wrow0 .. wrow0 + k)[0..n)), the kernels read weight columns >= n only into accumulator columns they never store."""
import os
import subprocess
import sys
import zlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -7.0                      # pre-fill of every output buffer
GX = 0.25                        # grid of the exact cases' inputs
ROUTE_SWITCHES = ('DET6D_ROWS_RESIDENT', 'DET6D_ROWS_RB', 'DET6D_ROWS_BLOCKS')


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- stacks: a chain is (k0, widths, {layer: options}); options: act (default 1 for hidden layers, 0 for the last), shift
# (False: NULL), wrow0, ldw (columns beyond n), store (ocol0 of a stored hidden layer / of the last layer), ldo ----
def chain(k0, *widths, **opts):
    return (k0, widths, {int(k[1:]): v for k, v in opts.items()})


TOWER3, TOWER32 = chain(512, 128, 3), chain(512, 128, 32)
#: group 1 of the issue; tests/test_host_logic.py asserts that det6d_mlp_rows_supported accepts every one of them
STACKS = {
    'G1-256x40': [chain(256, 40, l0=dict(act=1, ldw=4))],
    'G1-64x64x64x64x5': [chain(64, 64, 64, 64, 5, l0=dict(shift=False), l1=dict(act=0), l2=dict(store=3))],
    'G1-96x64x33': [chain(96, 64, 33, l0=dict(store=3, ldo=68), l1=dict(wrow0=3))],
    'G1-128x96x100': [chain(128, 96, 100, l0=dict(shift=False), l1=dict(shift=False, act=1))],
    'G1-64x32x257': [chain(64, 32, 257, l1=dict(ldw=5))],
    'G1-288x64x7': [chain(288, 64, 7, l0=dict(wrow0=3, act=0))],
    'G1-512x256x32': [chain(512, 256, 32, l0=dict(store=3))],
    'G1-992x256x32': [chain(992, 256, 32)],                       # 32 x (993 + 257) x 4 = 160 000 bytes: the largest that fits
    'GC-1024x128x32': [chain(1024, 128, 32, l0=dict(shift=False, store=3))],
    'GC-768x64x3': [chain(768, 64, 3, l0=dict(wrow0=3), l1=dict(ldw=5))],
    'GC-512x128x512x32': [chain(512, 128, 512, 32, l0=dict(act=0), l1=dict(store=3))],       # third layer reads 512 columns of XA
    'GC-512x100': [chain(512, 100, l0=dict(act=1, ldw=3))],
    'GC-512x128x3+512x64x64x32x1': [TOWER3, chain(512, 64, 64, 32, 1, l1=dict(store=0))],
    'G1-512x128x3+512x256x32': [TOWER3, chain(512, 256, 32)],    # one wide first layer: no chunking for either chain
}
ROWS1 = [1, 31, 32, 33, 95, 225]       # 225: eight tiles, ragged — three workgroups (DET6D_ROWS_BLOCKS=3) walk 3 + 3 + 2 of them


def sa1(n, store0=False, store1=False):
    """[96 -> 64 -> 32 -> n]: aggregation output at column 3 of 68-wide rows, confidence layer reading weight rows 3..66"""
    return [chain(96, 64, 32, n, l0=dict(store=3, ldo=68) if store0 else {}, l1=dict(wrow0=3, store=0) if store1 else dict(wrow0=3))]


def build_chain(rng, k0, widths, opts, kind):
    layers, k, grid = [], k0, GX
    for l, n in enumerate(widths):
        o = opts.get(l, {})
        last = l == len(widths) - 1
        L = SimpleNamespace(k=k, n=n, act=o.get('act', 0 if last else 1), wrow0=o.get('wrow0', 0), gw=1.0,
                            ocol0=o.get('store', 0 if last else None))
        if kind == 'exact':
            # c = max(8, ceil(k / n)) entries of +-1 per column, dealt round-robin over a permutation of the rows: every row is
            # used by some column; times 1 / 0.5 by layer parity
            c = max(8, -(-k // n))
            perm = rng.permutation(k)
            wl = np.zeros((k, n), np.float32)
            for j in range(n):
                wl[perm[(j * c + np.arange(c)) % k], j] = rng.choice([-1.0, 1.0], c)
            L.gw = 0.5 if l & 1 else 1.0
            wl *= L.gw
            grid *= L.gw
            shift = (rng.integers(-3, 4, n) * grid).astype(np.float32)
        else:
            wl = (rng.normal(size=(k, n)) / np.sqrt(k)).astype(np.float32)
            shift = rng.normal(size=(n,)).astype(np.float32)
        # a skipped k-block or column tile cannot hide behind zeros
        assert (wl != 0).any(axis=1).all() and (wl != 0).any(axis=0).all()
        L.wl, L.shift = wl, shift if o.get('shift', True) else None
        L.w = np.full((L.wrow0 + k + 1, n + o.get('ldw', 0)), np.nan, np.float32)
        L.w[L.wrow0:L.wrow0 + k, :n] = wl
        if L.ocol0 is not None:
            L.ldo = o.get('ldo', L.ocol0 + n + 2)
            assert L.ldo > L.ocol0 + n or L.ocol0 > 0
        layers.append(L)
        k = n
    return layers


def make_x(rng, rows, k0, kind):
    if kind == 'exact':
        return (rng.integers(-3, 4, (rows, k0)) * GX).astype(np.float32)
    return rng.normal(size=(rows, k0)).astype(np.float32)


def reference(kind, oracle_ops, x, layers):
    """the outputs of every layer of one chain"""
    outs = []
    if kind == 'oracle':
        h = x
        for L in layers:
            h = oracle_ops.linear(h, L.wl, L.shift, L.act)
            outs.append(h)
        return outs
    h, grid = x.astype(np.float64), GX
    for L in layers:
        w = L.wl.astype(np.float64)
        s = 0.0 if L.shift is None else L.shift.astype(np.float64)
        grid *= L.gw
        # every partial sum of every summation order is a multiple of `grid` below 2^24 grid: exact in fp32
        assert (np.abs(h) @ np.abs(w) + np.abs(s)).max() / grid < 2 ** 24
        y = h @ w + s
        assert (np.rint(y / grid) == y / grid).all()
        h = np.maximum(y, 0.0) if L.act else y
        outs.append(h.astype(np.float32))
        assert (outs[-1] == h).all()
    return outs


def place_x(x, xcol0=0, pad=0, off=0):
    """x as columns [xcol0, xcol0 + k0) of NaN rows of xcol0 + k0 + pad floats; off: a view `off` floats into a larger allocation"""
    rows, k0 = x.shape
    full = np.full((rows, xcol0 + k0 + pad), np.nan, np.float32)
    full[:, xcol0:xcol0 + k0] = x
    if not off:
        return dev(full)
    big = torch.full((full.size + 8,), float('nan'), device='cuda')
    view = big[off:off + full.size].view(full.shape)
    view.copy_(torch.from_numpy(full))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * off
    return view


def launch(chains, x_dev, xcol0, rows_alloc):
    """one det6d_mlp_rows over sentinel-filled outputs -> per chain, per layer: the whole output buffer (numpy) or None"""
    from de6d_amd.ops import fused
    specs, outs = [], []
    for layers in chains:
        spec = []
        for L in layers:
            out = None if L.ocol0 is None else torch.full((rows_alloc, L.ldo), SENT, device='cuda')
            spec.append((dev(L.w), L.wrow0, None if L.shift is None else dev(L.shift), L.k, L.n, L.act, out, L.ocol0 or 0))
        specs.append(spec)
    assert fused.mlp_rows_eligible(chains[0][0].k, specs)          # a case that fell back to per-layer launches fails here
    fused.mlp_rows(x_dev, xcol0, specs)
    torch.cuda.synchronize()
    for spec in specs:
        outs.append([None if l[6] is None else l[6].cpu().numpy() for l in spec])
    return outs


def compare(chains, outs, refs, rows, what):
    for c, layers in enumerate(chains):
        for l, L in enumerate(layers):
            if L.ocol0 is None:
                continue
            want = np.full(outs[c][l].shape, SENT, np.float32)
            want[:rows, L.ocol0:L.ocol0 + L.n] = refs[c][l]
            np.testing.assert_array_equal(outs[c][l], want, err_msg='%s: chain %d layer %d' % (what, c, l))


def check_case(oracle_ops, spec, rows, kind, what, xcol0=0, pad=0, off=0):
    rng = np.random.default_rng(zlib.crc32(('%s %d %s' % (what, rows, kind)).encode()))
    x = make_x(rng, rows, spec[0][0], kind)
    chains = [build_chain(rng, *c, kind) for c in spec]
    refs = [reference(kind, oracle_ops, x, layers) for layers in chains]
    outs = launch(chains, place_x(x, xcol0, pad, off), xcol0, rows + 3)
    compare(chains, outs, refs, rows, what)


# ---- 1. stack structures on the general routes ----
@pytest.mark.parametrize("kind", ["exact", "oracle"])
@pytest.mark.parametrize("rows", ROWS1)
@pytest.mark.parametrize("name", list(STACKS))
def test_stack_structures(oracle_ops, name, rows, kind):
    """depth 1 to 4, one and two chains, K-chunked inputs of 2 / 3 / 4 chunks, last widths with an edge column tile next to
    interior ones, stored hidden layers, hidden act = 0, last act = 1, shift = NULL, wrow0, ldw > n; up to a ragged third tile"""
    check_case(oracle_ops, STACKS[name], rows, kind, name)


@pytest.mark.parametrize("kind", ["exact", "oracle"])
def test_stack_above_the_default_lds_limit_on_one_device(oracle_ops, kind):
    """G1-480x256x32 over 64 rows: 94 464 bytes of LDS, above the 64 KB default and not K-chunked (test_compact_gpu.py runs this
    stack only where there are two devices)"""
    check_case(oracle_ops, [chain(480, 256, 32, l1=dict(act=1))], 64, kind, 'G1-480x256x32')


# ---- 2. input forms: must equal the aligned result ----
FORMS = {'xcol3-ldx+4': dict(xcol0=3, pad=1), 'xcol4': dict(xcol0=4, pad=4), 'odd-ldx': dict(pad=1), 'base+4B': dict(off=1),
         'xcol3-odd-ldx-base+4B': dict(xcol0=3, pad=2, off=1)}


@pytest.mark.parametrize("kind", ["exact", "oracle"])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name,spec", [('G1-96x64x32x1', sa1(1, True)), ('GC-512x128x3', [TOWER3])],
                         ids=['G1-96x64x32x1', 'GC-512x128x3'])
def test_input_forms(oracle_ops, name, spec, form, kind):
    """the scalar loader (production's vote FC reads columns 3.. of its rows; odd ldx; a base 4 bytes off 16-byte alignment) and
    the 16-byte loader at a column offset, 77 rows: the aligned launch's bits, which are the reference's"""
    f = dict(dict(xcol0=0, pad=0, off=0), **FORMS[form])
    rows = 77
    rng = np.random.default_rng(zlib.crc32(('%s %s' % (name, kind)).encode()))
    x = make_x(rng, rows, spec[0][0], kind)
    chains = [build_chain(rng, *c, kind) for c in spec]
    refs = [reference(kind, oracle_ops, x, layers) for layers in chains]
    aligned = launch(chains, place_x(x), 0, rows + 3)
    compare(chains, aligned, refs, rows, name + ' aligned')
    xd = place_x(x, f['xcol0'], f['pad'], f['off'])
    vec4 = xd.shape[1] % 4 == 0 and f['xcol0'] % 4 == 0 and xd.data_ptr() % 16 == 0
    assert vec4 == (form == 'xcol4')                                 # the loader this form is meant to take
    got = launch(chains, xd, f['xcol0'], rows + 3)
    for a, g in zip(aligned, got):
        for ya, yg in zip(a, g):
            if ya is not None:
                np.testing.assert_array_equal(yg, ya)


# ---- 3. no rows ----
@pytest.mark.parametrize("name", ['G1-96x64x33', 'GC-512x128x3+512x64x64x32x1'])
def test_no_rows_is_a_no_op(name):
    """rows = 0 (an empty tensor has no address): success, and no output element is written"""
    rng = np.random.default_rng(3)
    chains = [build_chain(rng, *c, 'oracle') for c in STACKS[name]]
    outs = launch(chains, place_x(np.zeros((0, chains[0][0].k), np.float32)), 0, 3)
    for per_chain in outs:
        for y in per_chain:
            assert y is None or (y == SENT).all()


# ---- 4. the persistent tile walk at default settings.  The launcher caps the grid at 256 x per_cu / nchains workgroups,
# per_cu = min(4, 160 KB / LDS of a tile); a workgroup takes a second tile only beyond that many tiles:
#   G1-480x256x32      32 x (481 + 257) x 4 = 94 464 bytes: per_cu 1, cap 256 tiles = 8 192 rows (k0 > 256: no input prefetch)
#   G1-128x96x100      32 x (129 + 97) x 4 = 28 928 bytes: per_cu 4, cap 1 024 tiles = 32 768 rows (input prefetched a tile ahead)
#   GC towers          K-chunks of 256: 32 x (257 + 129) x 4 = 49 408 bytes: per_cu 3, two chains: cap 384 tiles = 12 288 rows
#   G2-64x64x32x3      64-row tiles, 64 x (65 + 65) x 4 = 33 280 bytes: per_cu 4, cap 1 024 tiles = 65 536 rows; the last tile
#                      holds 8 rows: its second row block is empty
#   G1-640x64x3        a narrow stack over >= 16 384 rows whose 64-row tile (64 x (641 + 65) x 4 = 180 736 bytes) does not fit:
#                      32-row tiles (the launcher used to answer EINVAL for a stack det6d_mlp_rows_supported accepts)
WALKS = [('G1-480x256x32', [chain(480, 256, 32)], 8192 + 101, 'exact'),
         ('G1-128x96x100', [chain(128, 96, 100)], 32768 + 101, 'exact'),
         ('GC-512x128x3+512x128x32', [TOWER3, TOWER32], 12288 + 70, 'exact'),
         ('G2-64x64x32x3', [chain(64, 64, 32, 3, l1=dict(store=3))], 65536 + 200, 'exact'),
         ('G2-64x64x32x3', [chain(64, 64, 32, 3)], 16384 + 40, 'oracle'),
         ('G1-640x64x3', [chain(640, 64, 3)], 16384 + 33, 'exact')]


@pytest.mark.parametrize("name,spec,rows,kind", WALKS, ids=['%s-%d-%s' % (w[0], w[2], w[3]) for w in WALKS])
def test_persistent_walk(oracle_ops, name, spec, rows, kind):
    check_case(oracle_ops, spec, rows, kind, name)


# ---- 5. the SA1 routes: W (wave-private 32-row tiles, at most 512 workgroups of four: a wave takes a second tile beyond 2 048
# tiles = 65 536 rows; 16 384 + 5 x 32 rows end in a workgroup of one wave) and R (64-row tiles on at most 512 workgroups,
# double-buffered input: a second tile beyond 32 768 rows, a third beyond 65 536) ----
SA1_CASES = [('W', 16384, 1, True, False, 'oracle'), ('W', 16384, 1, True, False, 'exact'), ('W', 16384, 32, False, False, 'exact'),
             ('W', 16384 + 5 * 32, 7, True, True, 'exact'), ('W', 65536 + 7 * 32, 1, True, False, 'exact'),
             ('W', 65536 + 7 * 32, 32, False, True, 'exact'),
             ('R', 16385, 1, True, False, 'oracle'), ('R', 16385, 32, False, False, 'exact'), ('R', 16384 + 63, 7, True, True, 'exact'),
             ('R', 32768 + 3 * 64 + 17, 32, True, False, 'exact'), ('R', 70001, 1, True, False, 'exact'),
             ('R', 70001, 7, False, False, 'exact')]


@pytest.mark.parametrize("route,rows,n,store0,store1,kind", SA1_CASES,
                         ids=['%s-%d-n%d-%s%s%s' % (c[0], c[1], c[2], 'agg-' if c[3] else '', 'hid-' if c[4] else '', c[5]) for c in SA1_CASES])
def test_sa1_routes(oracle_ops, route, rows, n, store0, store1, kind):
    """[96 -> 64 -> 32 -> n], weight rows 3..66 in the second layer as production has them, with and without the stored
    aggregation output (column 3 of 68-wide rows) and the stored second layer"""
    assert (rows % 32 == 0) == (route == 'W') and rows >= 16384
    check_case(oracle_ops, sa1(n, store0, store1), rows, kind, 'sa1 n=%d' % n)


def test_sa1_wave_route_at_a_column_offset(oracle_ops):
    """W-xcol4: the 16-byte buffer loads of the wave-private kernel from columns 4..99 of 104-wide rows, partial last workgroup"""
    check_case(oracle_ops, sa1(7, True), 16384 + 5 * 32, 'exact', 'sa1 xcol0=4', xcol0=4, pad=4)


# ---- 6. the other routes of the same cases (experiments build; the switches are read once per process: child process) ----
@pytest.mark.parametrize("env,select", [
    ({'DET6D_ROWS_RESIDENT': '1'}, 'test_sa1_'),       # W's cases on the four-wave resident kernel
    ({'DET6D_ROWS_RESIDENT': '0'}, 'test_sa1_'),       # W's and R's cases on the general kernel (64-row tiles)
    ({'DET6D_ROWS_RB': '3'}, 'test_stack_structures or test_input_forms'),       # 64-row tiles whatever the row count
    ({'DET6D_ROWS_RB': '1'}, 'test_stack_structures or test_input_forms'),
    ({'DET6D_ROWS_BLOCKS': '3'}, 'test_stack_structures or test_input_forms')],  # three workgroups per chain walk all tiles
    ids=lambda v: '-'.join('%s=%s' % kv for kv in v.items()) if isinstance(v, dict) else v.replace(' ', '_'))
def test_other_routes(env, select):
    """same references, hence the same bits as the default route"""
    if any(k in os.environ for k in ROUTE_SWITCHES):
        pytest.skip('already a child')
    out = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-m', 'gpu', '-k', select],
                         env=dict(os.environ, DET6D_EXPERIMENTS_LIB='1', **env), cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert 'passed' in out.stdout
