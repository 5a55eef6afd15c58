"""Generate the P6 fixtures (G5) by running the REFERENCE itself (build container only, CPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_p6.py

Builds the reference ``Model`` from tests/p6_case.py's p6-mini config (IDetect and IAuxDetect
variants) and from its DownC block, loads ycx.utils.synth weights, sets ``stride`` on the head (the
reference leaves it None, as for G4) and records the eval outputs on a seeded image:

  tests/golden/g5_p6.npz    <variant>/z, <variant>/x<i>, downc/0
  tests/golden/g5_p6.json   layer count, save list, parameter count, state_dict key hash, seeds

Data only, no reference source. The other fixtures and manifest.json are not touched."""
from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402  (path set-up, import_reference, sd_hash)
import p6_case as P  # noqa: E402
from ycx.utils.synth import synthetic_images, synthetic_state_dict  # noqa: E402


def keys_hash(sd):
    return hashlib.sha256('\n'.join(sorted(sd.keys())).encode()).hexdigest()


def main():
    sys.path.insert(0, HERE)
    Model, _, _ = G.import_reference()
    torch.set_num_threads(8)
    arrays, meta = {}, {}
    x = synthetic_images(*P.SHAPE, seed=P.IMG_SEED)
    for name, head in P.VARIANTS.items():
        m = Model(P.p6_mini(head), P.ANCHORS4, P.NC).eval()
        sd = synthetic_state_dict(m, seed=P.W_SEED)
        m.load_state_dict(sd)
        m.model[-1].stride = torch.tensor(P.STRIDES)
        with torch.no_grad():
            z, xs = m(x)
        arrays[f'{name}/z'] = z.numpy().copy()
        for j, t in enumerate(xs):
            arrays[f'{name}/x{j}'] = t.numpy().copy()
        meta[name] = dict(head=head, nc=P.NC, shape=list(P.SHAPE), img_seed=P.IMG_SEED, w_seed=P.W_SEED,
                          strides=P.STRIDES, n_layers=len(m.model), save=list(m.save),
                          n_params=sum(p.numel() for p in m.parameters()), n_keys=len(sd), keys_sha256=keys_hash(sd),
                          sd_hash=G.sd_hash(sd), n_x=len(xs))
        print('G5', name, z.shape, [tuple(t.shape) for t in xs])
    m = Model(P.downc_block(), P.ANCHORS4, P.NC).eval()
    sd = synthetic_state_dict(m, seed=P.DOWNC_W_SEED)
    m.load_state_dict(sd)
    with torch.no_grad():
        y = m(synthetic_images(*P.DOWNC_SHAPE, seed=P.DOWNC_IMG_SEED))
    arrays['downc/0'] = y.numpy().copy()
    meta['downc'] = dict(shape=list(P.DOWNC_SHAPE), img_seed=P.DOWNC_IMG_SEED, w_seed=P.DOWNC_W_SEED,
                         n_keys=len(sd), keys_sha256=keys_hash(sd), sd_hash=G.sd_hash(sd))
    print('G5 downc', y.shape)
    np.savez_compressed(os.path.join(G.GOLD, 'g5_p6.npz'), **arrays)
    with open(os.path.join(G.GOLD, 'g5_p6.json'), 'w') as f:
        json.dump(meta, f, indent=1)
    print('bytes', os.path.getsize(os.path.join(G.GOLD, 'g5_p6.npz')) + os.path.getsize(os.path.join(G.GOLD, 'g5_p6.json')))


if __name__ == '__main__':
    main()
