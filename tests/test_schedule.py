"""Host-side (CPU) checks of ycx.schedule: the launches and buffers of every case of
tests/schedule_case.py against tests/golden/g7_schedule.json, which was recorded from the fusion
passes as Engine carried them before the schedule was a module of its own (the file's "parent"
commit; tests/golden/make_golden_schedule.py), and the properties every schedule keeps."""
import json
import os

import pytest

import schedule_case as C
from ycx.schedule import Schedule

CASES = C.cases()


@pytest.fixture(scope='module')
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g7_schedule.json')) as f:
        g = json.load(f)
    assert len(g['parent']) == 40 and list(g['cases']) == list(CASES)
    return g['cases']


@pytest.mark.parametrize('name', list(CASES))
def test_schedule_matches_the_recorded_one(name, golden, monkeypatch):
    net, shape, precision, off, env = CASES[name]
    for e in C.ENV:
        monkeypatch.delenv(e, raising=False)
    if env:
        monkeypatch.setenv(env, '1')
    plan = C.plan(net, shape)
    sched = Schedule(plan, precision, **{f: False for f in off})
    launches, buffers = C.encode(plan, sched)
    assert launches == golden[name]['launches']
    assert buffers == golden[name]['buffers']

    nodes = plan.graph.nodes
    index = {id(nd): i for i, nd in enumerate(nodes)}
    # every node is in exactly one launch: a concat in each of its copies, one without copies in none
    covered = [index[id(nd)] for la in sched.launches for nd in la.nodes]
    want = [i for i, nd in enumerate(nodes) for _ in range(len(nd.p['copies']) if nd.kind == 'concat' else 1)]
    assert sorted(covered) == want
    for la in sched.launches:
        if la.kind == 'copy':
            (nd,) = la.nodes
            assert nd.kind in ('up', 'concat', 'tonchw') and la.dst is nd.out and la.src in nd.inputs
    # launches run in the graph order of their first node
    first = [index[id(la.nodes[0])] for la in sched.launches]
    assert first == sorted(first)
    # no buffer is allocated twice
    assert len({id(b) for b in sched.activation_bufs}) == len(sched.activation_bufs)
