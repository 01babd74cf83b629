"""The oracle against the REFERENCE's own iou3d_cpu.cpp: its IoU matrices on these inputs are stored in
tests/golden/ref_iou.npz (make_golden.py: gen_ref_iou, from the library oracle/Makefile builds into oracle/_ref)."""
import os

import numpy as np
import pytest

from tests.util import random_boxes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_iou.npz')
CASES = [(1, 300, 30.0), (2, 128, 6.0), (3, 64, 2.0)]


def degenerate_boxes():
    boxes = random_boxes(9, 40, spread=5.0)
    boxes[1] = boxes[0]
    boxes[2, 3:5] = 0
    boxes[3, 6] = 0.0
    boxes[4, 6] = np.pi / 2
    boxes[5] = boxes[3]; boxes[5, 0] += boxes[3, 3]
    return boxes


@pytest.mark.parametrize("seed,k,spread", CASES)
def test_iou_matrix_and_keep_lists(oracle_ops, seed, k, spread):
    ref = np.load(GOLDEN)
    boxes = random_boxes(seed, k, spread=spread)
    np.testing.assert_array_equal(boxes, ref['boxes_%d' % seed])
    ours = oracle_ops.boxes_iou_bev(boxes, boxes)
    theirs = ref['iou_%d' % seed]
    np.testing.assert_allclose(ours, theirs, rtol=0, atol=2e-5)
    for thr in (0.01, 0.1, 0.5):
        np.testing.assert_array_equal(oracle_ops.nms(boxes, thr), oracle_ops.nms_from_iou(theirs, thr))


def test_degenerate_boxes(oracle_ops):
    ref = np.load(GOLDEN)
    boxes = degenerate_boxes()
    np.testing.assert_array_equal(boxes, ref['boxes_degenerate'])
    ours = oracle_ops.boxes_iou_bev(boxes, boxes)
    theirs = ref['iou_degenerate']
    np.testing.assert_allclose(ours, theirs, rtol=0, atol=2e-5)
