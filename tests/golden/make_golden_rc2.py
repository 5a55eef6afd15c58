"""Generate the RobustConv2 fixtures (G8) by running the REFERENCE itself (build container only, CPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rc2.py

Builds the reference ``Model`` from tests/rc2_case.py's rc2-mini config, loads its seeded weights
(``rc2_case.state_dict``: the synth recipe plus the transposed convs and an O(1) gamma), sets ``stride``
on the head (the reference leaves it None, as for G4 - G6) and records the eval outputs on a seeded image
and the builder's bookkeeping:

  tests/golden/g8_rc2.npz    x (the input), z, x<i>  (fp32)
  tests/golden/g8_rc2.json   layer count, save list, parameter count, state_dict key hash, seeds

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
import rc2_case as C  # noqa: E402
from make_golden_p6 import keys_hash  # noqa: E402
from ycx.utils.synth import synthetic_images  # noqa: E402


def main():
    sys.path.insert(0, HERE)
    Model, _, _ = G.import_reference()
    torch.set_num_threads(8)
    m = Model(C.rc2_mini(), C.ANCHORS2, C.NC).eval()
    sd = C.state_dict(m)
    m.load_state_dict(sd)
    m.model[-1].stride = torch.tensor(C.STRIDES)
    x = synthetic_images(*C.SHAPE, seed=C.IMG_SEED)
    with torch.no_grad():
        z, xs = m(x)
    arrays = {'x': x.numpy().copy(), 'z': z.numpy().copy()}
    for j, t in enumerate(xs):
        arrays[f'x{j}'] = t.numpy().copy()
    gammas = [float(v.abs().min()) for k, v in sd.items() if k.endswith('.gamma')]
    meta = dict(n_layers=len(m.model), save=list(m.save), n_params=sum(p.numel() for p in m.parameters()),
                n_keys=len(sd), keys_sha256=keys_hash(sd), nc=C.NC, shape=list(C.SHAPE), img_seed=C.IMG_SEED,
                w_seed=C.W_SEED, strides=C.STRIDES, sd_hash=G.sd_hash(sd), n_x=len(xs), min_abs_gamma=min(gammas))
    print('G8 rc2_mini', z.shape, [tuple(t.shape) for t in xs], 'min |gamma|', min(gammas))
    np.savez_compressed(os.path.join(G.GOLD, 'g8_rc2.npz'), **arrays)
    with open(os.path.join(G.GOLD, 'g8_rc2.json'), 'w') as f:
        json.dump(meta, f, indent=1)
    print('bytes', os.path.getsize(os.path.join(G.GOLD, 'g8_rc2.npz')) +
          os.path.getsize(os.path.join(G.GOLD, 'g8_rc2.json')))


if __name__ == '__main__':
    main()
