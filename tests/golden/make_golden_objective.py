"""Golden-vector generator of the CPN training objective (build container only: needs the reference checkout that
``oracle/ref_shim.py`` points to, which never travels).

Imports the read-only Python reference through ``oracle/ref_shim.py`` and builds ``CPN(backbone_stub, ..., core_cls=StubCore)``:
``StubCore.forward`` returns four leaf tensors in place of the network's heads.  After ``.train()``, ``model(x, targets=...)``
with ``full_detail=True`` returns the loss, the terms and the contours, and ``.backward()`` fills the gradients of the four
maps.  All of it runs on the CPU in float32.  Writes ``objective.npz`` next to this file: arrays only.

What the fixture pins is the reference's own code: ``CPN.forward`` and ``compute_loss`` (models/cpn.py:441-692),
``local_refinement`` (:63-85), ``fouriers2contours`` / ``scale_*`` / ``order_weighting`` / the bucket rules (ops/cpn.py),
``downsample_labels`` (ops/commons.py:51-78), ``iou_loss`` (ops/loss.py:90-110), the pairwise GIoU (ops/boxes.py:101-126),
``add_to_loss_dict`` / ``reduce_loss_dict`` (util/util.py:278-289) and torch's autograd through them.  ``torchvision`` is absent:
``box_area``, ``_upcast`` and ``remove_small_boxes`` are the three-line stand-ins of ``oracle/ref_shim.py``.

The inputs sit on coarse grids (maps are float16 values, refinement responses and target contours are multiples of 1 / 4), so that
equal minima, zero differences and values exactly on the clamp bounds occur, and so that the file stays small.  Every wrong
rule of ``tests/objective_oracle.py`` has to differ from the recorded result on at least one case (asserted below).

Run:  python tests/golden/make_golden_objective.py
"""
import os
import sys
import warnings
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
warnings.filterwarnings('ignore')

import objective_oracle as oracle  # noqa: E402

# name: dict(size, head, order, S, ...) -- everything else defaults as in ``make_case``
CASES = OrderedDict([
    ('base', dict(size=(32, 40), head=(16, 20), order=3, S=8)),
    ('nearest', dict(size=(35, 41), head=(18, 21))),
    ('stride4', dict(size=(32, 40), head=(8, 10))),
    ('order1', dict(order=1)),
    ('order1_plain', dict(order=1, order_weights=False)),
    ('order8', dict(order=8, S=16)),
    ('s1', dict(S=1)),
    ('s32', dict(S=32)),
    ('s65', dict(S=65, size=(12, 16), head=(6, 8))),
    ('buckets4', dict(buckets=4, S=8, linspace=True)),
    ('buckets4_random', dict(buckets=4, S=13)),
    ('classes4', dict(classes=4, class_targets=True)),
    ('classes4_default', dict(classes=4)),
    ('no_refinement', dict(refine=False, coef_scale=6.)),
    ('order_core', dict(order=3, order_core=5)),
    ('no_foreground', dict(empty_image=0)),
    ('no_proposals', dict(empty_image=(0, 1))),
    ('all_foreground', dict(full_image=0, size=(12, 16), head=(6, 8))),
    ('negative', dict(negative=.3)),
    ('outside', dict(coef_scale=9.)),
    ('thin', dict(thin=.5)),
    ('all_thin', dict(thin=1.)),
    ('order_weights_off', dict(order_weights=False)),
    ('weights', dict(weights=dict(fourier=.5, location=2., contour=1.5, score_bg=.25, score_fg=3., refinement=.75, iou=2.5))),
    ('iterations1', dict(iterations=1)),
])


def make_case(seed, size=(16, 20), head=(8, 10), order=3, S=8, order_core=None, buckets=1, classes=2, class_targets=False,
              refine=True, iterations=4, order_weights=True, weights=None, empty_image=(), full_image=None, negative=.08,
              coef_scale=2.5, thin=0., linspace=False, K=5, N=2):
    rng = np.random.RandomState(seed)
    H, W = size
    h, w = head
    order_core = order_core or order
    cs = 1 if classes <= 2 else classes

    def f16(a):
        return np.asarray(a, np.float16).astype(np.float32)

    labels = np.zeros((N, H, W), np.int64)
    for n in range(N):
        for k in rng.permutation(K)[:K - n]:  # the second image has one object fewer: a row of the targets stays unused
            cy, cx = rng.randint(0, H), rng.randint(0, W)
            ry, rx = rng.randint(2, max(3, H // 4)), rng.randint(2, max(3, W // 4))
            yy, xx = np.mgrid[:H, :W]
            labels[n][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = k + 1
        labels[n][(rng.rand(H, W) < negative) & (labels[n] > 0)] = -1
    for n in np.atleast_1d(empty_image):
        labels[n] = 0
    if full_image is not None:
        labels[full_image] = rng.randint(1, K + 1, (H, W))
    scale = np.ones((N, 1, h, w), np.float32)
    if thin:
        scale[rng.rand(N, 1, h, w) < thin] = .004
    maps = dict(scores=f16(rng.randn(N, cs, h, w) * 2),
                locations=f16(rng.randn(N, 2, h, w) * scale),
                fourier=f16(rng.randn(N, 4 * order_core, h, w) * coef_scale * scale /
                            np.repeat(np.arange(1, order_core + 1), 4)[None, :, None, None]),
                refinement=(np.round(rng.randn(N, 2 * buckets, H, W) * (.01 if thin else 1.5) * 4) / 4).astype(np.float32)
                if refine else None)
    if linspace:
        sampling = np.stack([torch.linspace(0, 1.0, S).numpy()] * N)  # the default sampling of ops.fouriers2contours
    else:
        sampling = np.sort(rng.uniform(0., 1., (N, S)), 1)
    centre = np.stack((rng.uniform(0, W, (N, K)), rng.uniform(0, H, (N, K))), -1)
    targets = dict(labels=labels,
                   fourier=f16(rng.randn(N, K, order, 4) * 3),
                   locations=f16(centre),
                   sampled_contours=(np.round((centre[:, :, None] + rng.randn(N, K, S, 2) * 5) * 4) / 4).astype(np.float32),
                   sampling=sampling.astype(np.float32))
    if class_targets:
        targets['classes'] = rng.randint(1, classes, (N, K)).astype(np.int64)
    config = dict(order=order, classes=classes, refine=refine, iterations=iterations, buckets=buckets,
                  order_weights=order_weights, weights=weights or {}, size=size)
    return maps, targets, config


def run_reference(rc, maps, targets, config):
    import torch.nn as nn
    leaves = {k: (None if v is None else torch.tensor(v, requires_grad=True)) for k, v in maps.items()}
    order_core = maps['fourier'].shape[1] // 4

    class StubCore(nn.Module):
        def __init__(self, **kwargs):
            super().__init__()
            self.order = order_core
            self.refinement_buckets = config['buckets']

        def forward(self, inputs):
            return leaves['scores'], leaves['locations'], leaves['refinement'], leaves['fourier'], None

    class Backbone(nn.Module):
        out_channels = [1, 1]

    S = targets['sampling'].shape[1]
    model = rc.CPN(Backbone(), order=config['order'], samples=S, classes=config['classes'], refinement=config['refine'],
                   refinement_iterations=config['iterations'], refinement_buckets=config['buckets'],
                   order_weights=config['order_weights'], core_cls=StubCore)
    model.weights.update(config['weights'])
    model.train()
    model.full_detail = True
    N = maps['scores'].shape[0]
    out = model(torch.zeros((N, 1) + tuple(config['size'])), targets={k: torch.as_tensor(v) for k, v in targets.items()})
    out['loss'].backward()
    rec = {'loss': out['loss'].detach().numpy()}
    for k, v in out['losses'].items():
        rec['term_' + k] = np.float32(np.nan) if v is None else v.detach().numpy()  # NaN: the term is None
        rec['none_' + k] = np.array(v is None)
    for k, v in leaves.items():
        if v is not None:
            rec['grad_' + k] = np.zeros(v.shape, np.float32) if v.grad is None else v.grad.numpy()
    rec['proposals'] = torch.cat(out['contour_proposals']).detach().numpy()
    rec['contours'] = torch.cat(out['contours']).detach().numpy()
    rec['boxes'] = torch.cat(out['boxes']).detach().numpy()
    return rec


def run_oracle(maps, targets, config, rules=()):
    ow = oracle.order_weighting(config['order']) if config['order_weights'] else None
    return oracle.objective(maps['scores'], maps['locations'], maps['refinement'], maps['fourier'], targets, config['size'],
                            config['order'], classes=config['classes'], refine=config['refine'], iterations=config['iterations'],
                            buckets=config['buckets'], order_weights=ow, weights=config['weights'], rules=rules)


def main():
    import ref_shim
    ref_shim.import_reference()
    import celldetection.models.cpn as rc

    out, caught = {}, {r: [] for r in oracle.WRONG_RULES}
    names = list(CASES)
    for i, name in enumerate(names):
        torch.manual_seed(i)
        maps, targets, config = make_case(100 + i, **CASES[name])
        rec = run_reference(rc, maps, targets, config)
        assert not oracle.departs(run_oracle(maps, targets, config), rec, print), f'{name}: the oracle departs from the reference'
        for rule in oracle.WRONG_RULES:
            if oracle.departs(run_oracle(maps, targets, config, (rule,)), rec):
                caught[rule].append(name)
        for k, v in maps.items():
            if v is not None:
                out[f'{name}/map_{k}'] = v.astype(np.float32 if k == 'refinement' else np.float16)
        for k, v in targets.items():
            out[f'{name}/target_{k}'] = v.astype(np.int16) if k == 'labels' else v
        for k, v in rec.items():
            out[f'{name}/{k}'] = v
        out[f'{name}/config'] = np.array([config['order'], config['classes'], int(config['refine']), config['iterations'],
                                          config['buckets'], int(config['order_weights'])] + list(config['size']), np.int64)
        wts = dict(oracle.DEFAULT_WEIGHTS)
        wts.update(config['weights'])
        out[f'{name}/weights'] = np.array([wts[k] for k in sorted(wts)], np.float64)
        print(name, 'P =', len(rec['boxes']), 'loss =', float(rec['loss']))
    for rule, where in caught.items():
        print(f'{rule}: caught on {where}')
        assert where, f'no case tells the wrong rule {rule} apart'
    out['names'] = np.array(names)
    path = os.path.join(HERE, 'objective.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
