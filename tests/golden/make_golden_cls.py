"""Generate the Classify / Rep-block fixtures (G13) by running the REFERENCE itself (build container only, CPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cls.py

Builds the reference ``Model`` from tests/cls_case.py's cls-mini and rep-mini configs and from each single
Rep block of its SINGLES table, loads ycx.utils.synth weights and records the eval output of the two networks
on a seeded image, with the builder's bookkeeping:

  tests/golden/g13_cls.npz    cls (2, 10) logits, rep (2, 64, 8, 8)
  tests/golden/g13_cls.json   per network and per single block: layer count, save list, parameter count,
                              state_dict key count and hash, sd_hash; the Classify module's state_dict keys
                              and shapes; seeds

Data only, no reference source. The other fixtures and manifest.json are not touched."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402  (path set-up, import_reference, sd_hash)
import cls_case as C  # noqa: E402
from make_golden_p6 import keys_hash  # noqa: E402
from ycx.utils.synth import synthetic_images, synthetic_state_dict  # noqa: E402


def book(m, sd):
    return dict(n_layers=len(m.model), save=list(m.save), n_params=sum(p.numel() for p in m.parameters()),
                n_keys=len(sd), keys_sha256=keys_hash(sd), sd_hash=G.sd_hash(sd))


def main():
    sys.path.insert(0, HERE)
    Model, _, _ = G.import_reference()
    torch.set_num_threads(8)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED)
    arrays, meta = {}, dict(shape=list(C.SHAPE), img_seed=C.IMG_SEED, w_seed=C.W_SEED, singles={})
    for name, cfg in (('cls', C.cls_mini()), ('rep', C.rep_mini())):
        m = Model(cfg, C.ANCHORS2, C.NC).eval()
        sd = synthetic_state_dict(m, seed=C.W_SEED)
        m.load_state_dict(sd)
        with torch.no_grad():
            y = m(x)
        arrays[name] = y.numpy().copy()
        meta[name] = dict(book(m, sd), out_shape=list(y.shape), out_absmax=float(y.abs().max()))
        if name == 'cls':
            head = m.model[-1]
            meta[name]['head_state_dict'] = {k: list(v.shape) for k, v in head.state_dict().items()}
            meta[name]['head_np'] = int(head.np)
    assert tuple(arrays['cls'].shape) == (C.SHAPE[0], C.CLS_C2) and tuple(arrays['rep'].shape) == C.REP_OUT
    for name, (module, args, c_in) in sorted(C.SINGLES.items()):
        m = Model(C.single(module, args, c_in), C.ANCHORS2, C.NC)
        meta['singles'][name] = dict(book(m, m.state_dict()), block_keys=list(m.model[-1].state_dict()))
        del meta['singles'][name]['sd_hash']  # random init: only the schema is recorded
    np.savez_compressed(os.path.join(G.GOLD, 'g13_cls.npz'), **arrays)
    with open(os.path.join(G.GOLD, 'g13_cls.json'), 'w') as f:
        json.dump(meta, f, indent=1)
    print('G13', {k: tuple(v.shape) for k, v in arrays.items()}, {k: meta[k]['out_absmax'] for k in ('cls', 'rep')})
    print('bytes', os.path.getsize(os.path.join(G.GOLD, 'g13_cls.npz')) +
          os.path.getsize(os.path.join(G.GOLD, 'g13_cls.json')))


if __name__ == '__main__':
    main()
