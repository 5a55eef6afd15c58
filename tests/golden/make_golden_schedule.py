"""Generate the schedule fixture (G7): the launch list and the buffer list of every case of
tests/schedule_case.py (CPU, no reference needed).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_schedule.py

  tests/golden/g7_schedule.json   {"parent": commit, "cases": {case id: {"launches", "buffers"}}}

The committed file was recorded at commit 66b2a91, before ``ycx.schedule`` existed, from the five
fusion passes and the launch ladder that ``Engine`` then carried ("parent" names that commit). This
script writes the same file through ``Schedule``; a diff after running it is a change of schedule.
One line per case. The other fixtures and manifest.json are not touched."""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for _p in (TESTS, os.path.join(os.path.dirname(TESTS), 'yolo-continuous_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import schedule_case as C  # noqa: E402

PATH = os.path.join(HERE, 'g7_schedule.json')
PARENT = '66b2a91fadcb80c1f10d6af4d771eca235bc520a'


def write(path, parent, record):
    """record(net, shape, precision, off, env) -> (launches, buffers)."""
    lines = []
    for name, case in C.cases().items():
        launches, buffers = record(*case)
        lines.append(json.dumps(name) + ': ' + json.dumps(dict(launches=launches, buffers=buffers),
                                                           separators=(',', ':')))
        print(name, len(launches), 'launches', len(buffers), 'buffers')
    with open(path, 'w') as f:
        f.write('{"parent": %s, "cases": {\n%s\n}}\n' % (json.dumps(parent), ',\n'.join(lines)))
    print('bytes', os.path.getsize(path))


def record(net, shape, precision, off, env):
    from ycx.schedule import Schedule
    for e in C.ENV:
        os.environ.pop(e, None)
    if env:
        os.environ[env] = '1'
    try:
        plan = C.plan(net, shape)
        return C.encode(plan, Schedule(plan, precision, **{f: False for f in off}))
    finally:
        os.environ.pop(env or '', None)


if __name__ == '__main__':
    write(PATH, PARENT, record)
