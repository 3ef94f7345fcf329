"""CPU: the launch sequence of every path of the host code -- each call into the kernels with the shapes and strides of its
tensors and the values of its scalars, recorded through the kernel emulation (tests/launch_trace.py) -- equals the pinned one
(tests/golden/launch_traces.json, written by tests/golden/make_launch_traces.py)."""
import json
import os

import pytest

from launch_trace import PATHS, summarise

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'launch_traces.json')) as f:
    PINNED = json.load(f)


def test_every_path_is_pinned():
    assert sorted(PINNED) == sorted(PATHS)


@pytest.mark.parametrize('path', list(PATHS))
def test_path_issues_the_pinned_launches(path):
    got, want = json.loads(json.dumps(summarise(PATHS[path]()))), PINNED[path]
    assert got['counts'] == want['counts']
    assert got['calls'] == want['calls'] and got['sha256'] == want['sha256']
