"""Generate the space/depth fixtures (G11) by running the REFERENCE itself (build container only, CPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_depth.py

Builds the reference ``Model`` from tests/depth_case.py's sd-mini config (Focus stem) and its plain-Conv-stem
variant, loads ycx.utils.synth weights, sets ``stride`` on the head (the reference leaves it None, as for
G4 / G5 / G6 / G9) and records the eval outputs on a seeded image; for both and for every one-block config
of ``SINGLES`` it also records the builder's bookkeeping:

  tests/golden/g11_depth.npz    z, x<i> (Focus stem), conv_z, conv_x<i> (Conv stem)
  tests/golden/g11_depth.json   layer count, save list, parameter count, state_dict key hash, seeds

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
import depth_case as C  # noqa: E402
from make_golden_p6 import keys_hash  # noqa: E402
from ycx.utils.synth import synthetic_images, synthetic_state_dict  # noqa: E402


def book(m, sd):
    return dict(n_layers=len(m.model), save=list(m.save), n_params=sum(p.numel() for p in m.parameters()),
                n_keys=len(sd), keys_sha256=keys_hash(sd))


def main():
    sys.path.insert(0, HERE)
    Model, _, _ = G.import_reference()
    torch.set_num_threads(8)
    arrays, meta = {}, {'singles': {}}
    for stem, key, prefix in (('focus', 'sd_mini', ''), ('conv', 'sd_mini_conv', 'conv_')):
        m = Model(C.sd_mini(stem), C.ANCHORS2, C.NC).eval()
        sd = synthetic_state_dict(m, seed=C.W_SEED)
        m.load_state_dict(sd)
        m.model[-1].stride = torch.tensor(C.STRIDES)
        with torch.no_grad():
            z, xs = m(synthetic_images(*C.SHAPE, seed=C.IMG_SEED))
        arrays[prefix + 'z'] = z.numpy().copy()
        for j, t in enumerate(xs):
            arrays[f'{prefix}x{j}'] = t.numpy().copy()
        meta[key] = dict(book(m, sd), nc=C.NC, shape=list(C.SHAPE), img_seed=C.IMG_SEED, w_seed=C.W_SEED,
                         strides=C.STRIDES, sd_hash=G.sd_hash(sd), n_x=len(xs))
        print('G11', key, z.shape, [tuple(t.shape) for t in xs])
    for name, (module, args, c_in, _) in C.SINGLES.items():
        s = Model(C.single(module, args, c_in), C.ANCHORS2, C.NC)
        meta['singles'][name] = book(s, s.state_dict())
    s = Model(C.on_input('Focus', [32, 3]), C.ANCHORS2, C.NC)
    meta['singles']['Focus_on_input'] = book(s, s.state_dict())
    np.savez_compressed(os.path.join(G.GOLD, 'g11_depth.npz'), **arrays)
    with open(os.path.join(G.GOLD, 'g11_depth.json'), 'w') as f:
        json.dump(meta, f, indent=1)
    print('bytes', os.path.getsize(os.path.join(G.GOLD, 'g11_depth.npz')) +
          os.path.getsize(os.path.join(G.GOLD, 'g11_depth.json')))


if __name__ == '__main__':
    main()
