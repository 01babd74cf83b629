"""The entry points a pass calls, with their arguments, in their order, equal the traces recorded before the SA-layer refactor
(tests/launch_trace.py; tests/traces/*.json).  No GPU: the launches are stubbed, the route queries go to the real library."""
import os

import pytest

from tests import launch_trace


@pytest.fixture(scope='module')
def experiments_build():
    from de6d_amd import _build
    _build.build(experiments=True)


def test_every_case_has_its_fixture():
    have = sorted(f[:-5] for f in os.listdir(launch_trace.TRACE_DIR) if f.endswith('.json'))
    assert have == sorted(launch_trace.CASES)


@pytest.mark.parametrize('name', sorted(launch_trace.CASES))
def test_launch_trace(name, experiments_build):
    got, want = launch_trace.trace_of(name), launch_trace.fixture(name)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "launch %d of %s" % (i, name)
    assert len(got) == len(want), ([e[0] for e in got], [e[0] for e in want])
