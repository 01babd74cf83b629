"""The first-layer gather of the group kernels (csrc/mlp_group.hip: group_layer1, the list entries requested a tile ahead, the
ticket drawn behind the gather) on lists the other group tests do not reach: at their shapes every workgroup has at most one
tile of a compact list, so nothing there walks from a tile to the next.  Everything == the dense oracle's three layers over
ALL nsample rows, bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

from tests.test_compact_gpu import build_list, dev, make_layers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USAGE = os.path.join(ROOT, "de6d_amd", "csrc", "libdet6d_hip.usage.json")

#: (c_in, widths) -> workgroups per CU of the persistent grid (group_grid() in csrc/mlp_group.hip: by LDS, four at the most)
WIDTH_SETS = {(128, (128, 128, 256)): 4, (128, (128, 256, 256)): 3, (256, (256, 256, 512)): 2, (256, (256, 512, 1024)): 2}
PCOL0 = 8          # this group's sums at column 8 of a wider P


def full_rows(idx, cnt, ns):
    """the reference's padding: a ball with cnt hits repeats them periodically; an empty one holds zeros"""
    out = np.zeros_like(idx)
    for bi in range(idx.shape[0]):
        for j in range(idx.shape[1]):
            c = int(cnt[bi, j])
            if c:
                out[bi, j] = np.resize(np.sort(idx[bi, j, :c]), ns)
    return out


class Case:
    """inputs of one group launch and the oracle's pooled features for them"""

    def __init__(self, oracle_ops, c_in, widths, cnt, idx, n, seed):
        from de6d_amd.ops import fused
        b, m, ns = idx.shape
        rng = np.random.default_rng(seed)
        ld = (3 + c_in + 3) // 4 * 4
        rows = np.zeros((b, n, ld), np.float32)
        rows[..., :3 + c_in] = rng.normal(size=(b, n, 3 + c_in))
        ctr = rng.normal(size=(b, m, 3)).astype(np.float32)
        layers_np, self.layers = make_layers(rng, ld, c_in, widths)
        h = oracle_ops.linear(rows, layers_np[0][0], layers_np[0][1], 1, idx=idx, ctr=ctr)
        h = oracle_ops.linear(h, layers_np[1][0], layers_np[1][1], 1)
        self.ref = oracle_ops.linear(h, layers_np[2][0][:, :widths[2]], layers_np[2][1], 1, cnt=cnt, pool=ns)
        self.rows, self.ctr = dev(rows), dev(ctr)
        wz = self.layers[0][0].clone()
        wz[:3] = 0
        self.p = torch.empty((b * n, wz.shape[1] + 2 * PCOL0), device="cuda")
        fused.linear(self.rows.view(b * n, ld), wz, None, 0, self.p, col0=PCOL0)
        self.cr = build_list(fused, cnt, idx, n, 1, 1)
        self.shape = (b * m, widths[2])

    def launch(self):
        from de6d_amd.ops import fused
        out = torch.zeros(self.shape, device="cuda")
        fused.mlp_group3(self.p, PCOL0, self.layers, self.rows, self.ctr, out, 0, compact=self.cr)
        return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("c_in,widths", list(WIDTH_SETS))
def test_more_live_tiles_than_the_persistent_grid(oracle_ops, c_in, widths):
    """every ball full, nsample 32: one tile per centre, eight centres more than 256 CUs x workgroups per CU, so some
    workgroups walk on to a tile drawn by ticket, with its list entries requested a tile ahead.  The same list launched twice:
    the ticket pair cleans itself, the same bits both times."""
    b, n, ns = 2, 300, 32
    m = (256 * WIDTH_SETS[(c_in, widths)] + 8) // b
    rng = np.random.default_rng(sum(widths))
    cnt = np.full((b, m), ns, np.int32)
    idx = np.sort(rng.permuted(np.tile(np.arange(n, dtype=np.int32), (b, m, 1)), axis=2)[..., :ns], axis=2)
    case = Case(oracle_ops, c_in, widths, cnt, idx, n, 11)
    hdr = case.cr.hdr.cpu().numpy()
    assert hdr[0] // 32 == b * m > 256 * WIDTH_SETS[(c_in, widths)]
    first = case.launch()
    np.testing.assert_array_equal(case.cr.hdr.cpu().numpy()[10:12], 0)       # ticket and exit counter
    np.testing.assert_array_equal(first, case.ref)
    np.testing.assert_array_equal(case.launch(), case.ref)
    np.testing.assert_array_equal(case.cr.hdr.cpu().numpy()[10:12], 0)


@pytest.mark.gpu
@pytest.mark.parametrize("c_in,widths", [k for k in WIDTH_SETS if k[1] != (128, 256, 256)])
@pytest.mark.parametrize("kind", ["all_empty", "all_full", "all_single", "one_centre"])
def test_degenerate_lists_of_the_other_width_sets(oracle_ops, kind, c_in, widths):
    """the lists of test_compact_gpu.test_group_kernel_on_degenerate_lists; one_centre: a tile that requests its own entries
    again"""
    b, n, ns = 2, 300, 32
    m = 1 if kind == "one_centre" else 64
    rng = np.random.default_rng(5)
    cnt = {"all_empty": np.zeros((b, m)), "all_full": np.full((b, m), ns), "all_single": np.ones((b, m)),
           "one_centre": np.full((b, m), 21)}[kind].astype(np.int32)
    idx = full_rows(rng.integers(0, n, (b, m, ns)).astype(np.int32), cnt, ns)
    case = Case(oracle_ops, c_in, widths, cnt, idx, n, 6)
    np.testing.assert_array_equal(case.launch(), case.ref)


@pytest.mark.gpu
@pytest.mark.parametrize("c_in,widths", list(WIDTH_SETS))
def test_last_tile_of_a_class_is_one_row_and_alignment_rows(oracle_ops, c_in, widths):
    """97 single-hit centres, the last centre among them: their class fills three tiles and ONE row of a fourth, whose 31
    alignment rows (tag -1, list entry unspecified) gather row 0 and write zeros"""
    b, n, m, ns = 2, 300, 100, 32
    rng = np.random.default_rng(9)
    cnt = np.full((b, m), ns, np.int32)
    single = np.concatenate([rng.choice(b * m - 1, 96, replace=False), [b * m - 1]])
    cnt.reshape(-1)[single] = 1
    idx = full_rows(np.sort(rng.permuted(np.tile(np.arange(n, dtype=np.int32), (b, m, 1)), axis=2)[..., :ns], axis=2), cnt, ns)
    case = Case(oracle_ops, c_in, widths, cnt, idx, n, 10)
    hdr = case.cr.hdr.cpu().numpy()
    wide = -(-(b * m - 97) * 32 // 128) * 128                           # the class-32 region, padded to 128 rows
    assert hdr[1] == hdr[5] == wide and hdr[6] == hdr[0] == wide + 128    # class 1: the last 128 rows
    tags = case.cr.crow_c.cpu().numpy()[:hdr[0]]
    assert (tags[-128:] >= 0).sum() == 97 and tags[-32] >= 0 and (tags[-31:] == -1).all()
    np.testing.assert_array_equal(case.launch(), case.ref)


#: kernels of the default route (mangled-name fragments, %d = COMPACT) -> waves per SIMD the build before this gather held
DEFAULT_ROUTE = {"mlp_group_stream_kernelILi256ELi512ELi1024ELb%dEE": 2, "mlp_group_stream_kernelILi256ELi256ELi512ELb%dEE": 3,
                 "mlp_group_kernelILi128ELi128ELi256ELb%dELi4EE": 3, "mlp_group_kernelILi128ELi256ELi256ELb%dELi4EE": 3}


def test_group_kernels_keep_their_registers_and_residency():
    """the batch of requests is paid in registers: no group kernel may spill or touch scratch for it, and the instantiations of
    the default route keep their waves per SIMD"""
    if not os.path.exists(USAGE):
        pytest.skip("library not built by de6d_amd._build in this tree")
    with open(USAGE) as f:
        kernels = json.load(f)["mlp_group.hip"]
    assert len(kernels) >= 20
    for name, u in kernels.items():
        assert not u.get("ScratchSize", 0) and not u.get("VGPRs Spill", 0), (name, u)
    for frag, waves in DEFAULT_ROUTE.items():
        for compact in (0, 1):
            hit = [u for name, u in kernels.items() if frag % compact in name]
            assert len(hit) == 1, frag % compact
            assert hit[0]["Occupancy"] >= waves, (frag % compact, hit[0])

