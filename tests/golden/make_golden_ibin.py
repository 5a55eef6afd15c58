"""Generate the IBin fixtures (G12) by running the REFERENCE itself (build container only, CPU).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ibin.py

Builds the reference ``Model`` from tests/ibin_case.py's ibin-mini config, loads ycx.utils.synth weights,
sets ``stride`` on the head (the reference leaves it None, as for G4 / G5 / G11) and records the eval
outputs on a seeded image, with the builder's bookkeeping and the head module's state_dict schema:

  tests/golden/g12_ibin.npz    z (2, 240, nc + 5), x0 (2, 3, 8, 8, 50), x1 (2, 3, 4, 4, 50)
  tests/golden/g12_ibin.json   layer count, save list, parameter count, state_dict key hash, the head's
                               state_dict keys and shapes, seeds, sd_hash, and how many rows of z the end-to-end
                               test skips (top-two bin logits closer than the f32 bar: at most 1 %)

Data only, no reference source. The other fixtures and manifest.json are not touched."""
from __future__ import annotations

import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as G  # noqa: E402  (path set-up, import_reference, sd_hash)
import ibin_case as C  # noqa: E402
from make_golden_p6 import keys_hash  # noqa: E402
from ycx.utils.synth import synthetic_images, synthetic_state_dict  # noqa: E402

F32_TOL = 1e-3  # TOL['f32'] of tests/test_gpu_p6.py


def near_tie_rows(xs, tol=F32_TOL):
    """Per level, the (n, na, ny, nx) mask of rows whose top-two bin logits, for w or for h, are closer
    than ``tol`` times the row's largest |logit| (tests/test_gpu_ibin.py skips w / h there)."""
    masks = []
    for x in xs:
        scale = x.abs().amax(-1) * tol
        m = torch.zeros(x.shape[:-1], dtype=torch.bool)
        for lo in (3, 4 + C.BIN_COUNT):
            top = x[..., lo:lo + C.BIN_COUNT].topk(2, -1).values
            m |= (top[..., 0] - top[..., 1]) < scale
        masks.append(m)
    return masks


def main():
    sys.path.insert(0, HERE)
    Model, _, _ = G.import_reference()
    torch.set_num_threads(8)
    warnings.simplefilter('ignore')  # torch.range's deprecation notice, once per SigmoidBin
    m = Model(C.ibin_mini(), C.ANCHORS2, C.NC).eval()
    sd = synthetic_state_dict(m, seed=C.W_SEED)
    m.load_state_dict(sd)
    head = m.model[-1]
    head.stride = torch.tensor(C.STRIDES)
    with torch.no_grad():
        z, xs = m(synthetic_images(*C.SHAPE, seed=C.IMG_SEED))
    assert tuple(z.shape) == (C.SHAPE[0], sum(C.ROWS), C.NZ) and head.no == C.NO
    arrays = {'z': z.numpy().copy()}
    for j, t in enumerate(xs):
        arrays[f'x{j}'] = t.numpy().copy()
    skipped = sum(int(k.sum()) for k in near_tie_rows(xs))
    rows = C.SHAPE[0] * sum(C.ROWS)
    assert skipped <= 0.01 * rows, (skipped, rows)  # the golden itself leaves at most 1 % of the rows out
    meta = dict(n_layers=len(m.model), save=list(m.save), n_params=sum(p.numel() for p in m.parameters()),
                n_keys=len(sd), keys_sha256=keys_hash(sd),
                head_state_dict={k: list(v.shape) for k, v in head.state_dict().items()},
                nc=C.NC, no=int(head.no), bin_count=int(head.bin_count), shape=list(C.SHAPE), img_seed=C.IMG_SEED,
                w_seed=C.W_SEED, strides=C.STRIDES, sd_hash=G.sd_hash(sd), n_x=len(xs),
                near_tie_rows=skipped, rows=rows)
    np.savez_compressed(os.path.join(G.GOLD, 'g12_ibin.npz'), **arrays)
    with open(os.path.join(G.GOLD, 'g12_ibin.json'), 'w') as f:
        json.dump(meta, f, indent=1)
    print('G12 ibin_mini', tuple(z.shape), [tuple(t.shape) for t in xs], 'near-tie rows', skipped, 'of', rows)
    print('bytes', os.path.getsize(os.path.join(G.GOLD, 'g12_ibin.npz')) +
          os.path.getsize(os.path.join(G.GOLD, 'g12_ibin.json')))


if __name__ == '__main__':
    main()
