"""Generate the packing fixture (G10): the ops, descriptors, op_info and packed-tensor hashes of every case
of tests/pack_case.py, from an Engine bound to CPU memory (no GPU, no reference needed).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pack.py

  tests/golden/g10_pack.json   {"parent": commit, "table": [every distinct row],
                                "cases": {case id: {"ops", "packed", "conv_flops", ...}, rows by index}}

The committed file was recorded at commit 2a9505c, before ``ycx.pack`` existed, from the four packers and
hand-filled descriptors that ``Engine`` then carried ("parent" names that commit). This script writes the
same file through ``ycx.pack``; a diff after running it is a change of a packed byte, a descriptor field
or an op. One line per case, after the table of rows. The other fixtures and manifest.json are not touched."""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for _p in (TESTS, os.path.join(os.path.dirname(TESTS), 'yolo-continuous_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import pack_case as C  # noqa: E402

PATH = os.path.join(HERE, 'g10_pack.json')
PARENT = '2a9505c67b26ea9935181a07c85d02ae84e3fb71'


def record(net, shape, precision, no_silu_ps):
    from ycx import engine
    old = engine._NO_SILU_PS
    engine._NO_SILU_PS = no_silu_ps
    try:
        return C.encode(C.cpu_engine(C.plan(net, shape), precision))
    finally:
        engine._NO_SILU_PS = old


def write(path, parent):
    lines, table = [], {}
    for name, case in C.cases().items():
        enc = record(*case)
        lines.append(json.dumps(name) + ': ' + json.dumps(C.squeeze(enc, table), separators=(',', ':')))
        print(name, len(enc['ops']), 'ops', len(enc['packed']), 'packed tensors')
    rows = list(table)  # in index order; 64 to a line
    chunks = [','.join(rows[i:i + 64]) for i in range(0, len(rows), 64)]
    with open(path, 'w') as f:
        f.write('{"parent": %s, "table": [\n%s\n], "cases": {\n%s\n}}\n'
                % (json.dumps(parent), ',\n'.join(chunks), ',\n'.join(lines)))
    print(len(rows), 'distinct rows; bytes', os.path.getsize(path))


if __name__ == '__main__':
    write(PATH, PARENT)
