"""Times cda.CPNObjective (forward plus gradients of the four head maps) on one MI355X against the same rule written in stock
torch operations on the same GPU (forward plus ``backward()``), and prints one JSON line per workload.
    python tools/objective_microbench.py [repeats=10] [n=8] [side=512] [stride=2]

Workloads: ``n`` images of ``side`` x ``side`` with 64 discs each (about 19 % foreground: about 10^5 foreground head pixels at the
defaults), order 5, 4 refinement iterations, samples 32 and 64, refinement buckets 1 and 6.  Every time is the median of
``repeats`` device-event measurements after two warm-up calls; the whole list is printed next to it.  Both sides start from the
same tensors on the GPU and end with the gradients of the four maps; the losses of the two are compared (float32 sums in
different orders: a relative difference of about 1e-6 is expected)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import celldetection_amd as cda  # noqa: E402


def event_ms(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return round(float(np.median(times)), 3), [round(t, 3) for t in times], r


def workload(n, side, stride, order, samples, buckets, dev, seed=0):
    rng = np.random.RandomState(seed)
    H = W = side
    h, w = H // stride, W // stride
    grid, K = 8, 64
    pitch = side / grid
    radius = pitch * .25
    yy, xx = np.mgrid[:H, :W]
    labels = np.zeros((n, H, W), np.int32)
    centre = np.zeros((n, K, 2), np.float32)
    for i in range(n):
        for k in range(K):
            cy, cx = (k // grid + .5) * pitch + rng.uniform(-4, 4), (k % grid + .5) * pitch + rng.uniform(-4, 4)
            labels[i][(yy - cy) ** 2 + (xx - cx) ** 2 <= radius ** 2] = k + 1
            centre[i, k] = cx, cy
    sampling = np.sort(rng.uniform(0, 1, (n, samples)), 1).astype(np.float32)
    angle = 2 * np.pi * sampling[:, None, :, None]
    circle = np.concatenate((np.cos(angle), np.sin(angle)), -1) * radius
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32)).to(dev)
    targets = dict(labels=torch.as_tensor(labels).to(dev), fourier=t(rng.randn(n, K, order, 4)), locations=t(centre),
                   sampled_contours=t(centre[:, :, None] + circle), sampling=t(sampling))
    maps = dict(scores=t(rng.randn(n, 1, h, w)), locations=t(rng.randn(n, 2, h, w)),
                refinement=t(rng.randn(n, 2 * buckets, H, W)),
                fourier=t(rng.randn(n, 4 * order, h, w) * 3 / np.repeat(np.arange(1, order + 1), 4)[None, :, None, None]))
    return maps, targets, (H, W)


def torch_objective(maps, targets, size, order, buckets, iterations, order_weights, wts):
    """The rule of include/cpn_hip.h ("Training objective") in stock tensor operations; autograd gives the gradients."""
    import torch.nn.functional as F
    scores, locations, refinement, fourier = (maps[k] for k in ('scores', 'locations', 'refinement', 'fourier'))
    H, W = size
    N, _, h, w = fourier.shape
    dev = fourier.device
    lab = targets['labels'][:, None].float()
    if (H, W) != (h, w):
        lab = F.max_pool2d(lab, (H // h, W // w), (H // h, W // w))
        if lab.shape[-2:] != (h, w):
            lab = F.interpolate(lab, (h, w), mode='nearest')
    lab = lab[:, 0]
    b, y, x = torch.where(lab > 0)
    bb, by, bx = torch.where(lab == 0)
    rows = lab[b, y, x].long() - 1
    score = 0.
    if len(b):
        z = scores[b, 0, y, x]
        score = score + F.binary_cross_entropy_with_logits(z, torch.ones_like(z)) * wts['score_fg']
    if len(bb):
        z = scores[bb, 0, by, bx]
        score = score + F.binary_cross_entropy_with_logits(z, torch.zeros_like(z)) * wts['score_bg']
    coef = fourier.view(N, -1, 4, h, w)[b, :order, :, y, x]
    loc = locations[b, :, y, x] + torch.stack((x, y), 1).float()
    t = targets['sampling'][b]
    arg = float(np.pi) * 2 * torch.arange(1, order + 1, device=dev)[:, None] * t[:, None, :]
    con = loc[:, None, :] + (coef[:, :, None, (1, 3)] * torch.sin(arg)[..., None]).sum(1)
    con = con + (coef[:, :, None, (0, 2)] * torch.cos(arg)[..., None]).sum(1)
    scale = torch.tensor([W / w, H / h], dtype=torch.float32, device=dev)
    hi = torch.tensor([W - 1, H - 1], dtype=torch.float32, device=dev)
    lo = torch.zeros_like(hi)  # clamp with tensor bounds passes the gradient on the closed range, like clamp_
    con = con * scale
    coef = coef * scale.repeat_interleave(2)
    loc = loc * scale
    c_tar = targets['sampled_contours'][b, rows]
    terms = dict(fourier=((coef - targets['fourier'][b, rows]).abs() * order_weights).mean() * wts['fourier'],
                 location=(loc - targets['locations'][b, rows]).abs().mean() * wts['location'],
                 contour=(con - c_tar).abs().mean() * wts['contour'], score=score)
    cur, refined = con, 0.
    for _ in range(iterations):
        r = torch.minimum(torch.clamp(torch.round(cur.detach()), min=0), hi)
        ix, iy = r[..., 0].long(), r[..., 1].long()
        if buckets == 1:
            resp = refinement[b[:, None], :, iy, ix]
        else:
            base = t * buckets
            whole = base.long()
            resp = 0.
            for j in (whole - 1, whole, whole + 1):
                dist = (j + .5 - base).abs()
                wk = torch.where(dist > 1, torch.zeros_like(dist), 1. - dist)
                ch = (j % buckets) * 2
                resp = resp + refinement[b[:, None, None], torch.stack((ch, ch + 1), -1), iy[..., None], ix[..., None]] * wk[..., None]
        cur = r + resp
        refined = refined + (torch.clamp(cur, lo, hi) - c_tar).abs().mean() * wts['refinement']
    last = torch.clamp(cur, lo, hi)
    terms['refinement'] = refined
    box = torch.cat((last.min(1).values, last.max(1).values), 1)
    tbox = torch.cat((c_tar.min(1).values, c_tar.max(1).values), 1)
    keep = ((box[:, 2] - box[:, 0]) >= 1) & ((box[:, 3] - box[:, 1]) >= 1)
    box, tbox = box[keep], tbox[keep]
    area = lambda q: (q[:, 2] - q[:, 0]) * (q[:, 3] - q[:, 1])
    inter = (torch.minimum(box[:, 2:], tbox[:, 2:]) - torch.maximum(box[:, :2], tbox[:, :2])).clamp(min=0).prod(1)
    union = area(box) + area(tbox) - inter
    enc = (torch.maximum(box[:, 2:], tbox[:, 2:]) - torch.minimum(box[:, :2], tbox[:, :2])).clamp(min=0).prod(1)
    terms['iou'] = torch.nan_to_num((1 - (inter / union - (enc - union) / enc)).mean(), 0., 0., 0.) * wts['iou']
    return sum(terms[k] for k in ('fourier', 'location', 'contour', 'score', 'refinement', 'iou')), terms


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    side = int(sys.argv[3]) if len(sys.argv) > 3 else 512
    stride = int(sys.argv[4]) if len(sys.argv) > 4 else 2
    dev = torch.device('cuda:0')
    order, iterations = 5, 4
    for buckets in (1, 6):
        for samples in (32, 64):
            maps, targets, size = workload(n, side, stride, order, samples, buckets, dev)
            obj = cda.CPNObjective(order, samples, refinement_iterations=iterations, refinement_buckets=buckets)
            ow = obj.order_weights.to(dev)

            def leaves():
                return {k: v.clone().requires_grad_() for k, v in maps.items()}

            def ours():
                m = leaves()
                loss, _ = obj(m['scores'], m['locations'], m['refinement'], m['fourier'], targets, size=size)
                loss.backward()
                return loss.detach(), m

            def stock():
                m = leaves()
                loss, _ = torch_objective(m, targets, size, order, buckets, iterations, ow, obj.weights)
                loss.backward()
                return loss.detach(), m

            def clones():
                return leaves()

            c_ms, _, _ = event_ms(clones, repeats)
            o_ms, o_all, (o_loss, o_maps) = event_ms(ours, repeats)
            s_ms, s_all, (s_loss, s_maps) = event_ms(stock, repeats)
            P = int((torch.nn.functional.max_pool2d(targets['labels'][:, None].float(), stride, stride) > 0).sum())
            diff = {k: float((o_maps[k].grad - s_maps[k].grad).abs().max() / s_maps[k].grad.abs().max()) for k in maps}
            print(json.dumps(dict(n=n, side=side, stride=stride, order=order, iterations=iterations, samples=samples, buckets=buckets,
                                  proposals=P, objective_ms=o_ms, objective_ms_all=o_all, stock_torch_ms=s_ms, stock_torch_ms_all=s_all,
                                  clone_of_the_maps_ms_in_both=c_ms, stock_over_objective=round(s_ms / o_ms, 2),
                                  loss=float(o_loss), stock_loss=float(s_loss),
                                  largest_gradient_difference_over_largest_gradient=diff)), flush=True)


if __name__ == '__main__':
    main()
