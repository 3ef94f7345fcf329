"""`launch_traces.json`: for every path of tests/launch_trace.py (forward, backward, Trainer.step, greedy, the beam searches
(the reference's, n-best, stochastic, constrained by words and by phrases, ensemble with and without groups), sampling, SCST, Decoder.forward on its own, for the three model classes) the calls the host code makes into the kernels -- number
of calls, calls per op, SHA-256 of the detailed trace (op names in order, shapes, strides, scalars) -- recorded through the kernel
emulation.  The paths use the public API only: the fixture pins the launch sequence of the commit it was generated on,
and a refactor of the host code is checked against it (tests/test_launch_traces.py).  Regenerate it only for a launch that is
meant to change, and review the diff."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'd-lsg-video-caption_amd'), os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)


def dump(traces, path):
    """one line per path"""
    with open(path, 'w') as f:
        f.write('{\n' + ',\n'.join(' %s: %s' % (json.dumps(k), json.dumps(e, separators=(',', ':'))) for k, e in traces.items()) + '\n}\n')


if __name__ == '__main__':
    from launch_trace import record_all
    out = os.path.join(HERE, 'launch_traces.json')
    traces = record_all()
    dump(traces, out)
    print('%d paths, %d calls, %d bytes' % (len(traces), sum(e['calls'] for e in traces.values()), os.path.getsize(out)))
