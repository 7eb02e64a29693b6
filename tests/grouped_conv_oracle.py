"""fp64 statements of the trainable grouped 3x3 convolution (test helper, not a conftest): what csrc/grouped_conv_train.hip and
celldetection_amd/nn/grouped.py must compute, written index by index from the "Trainable grouped convolution" section
of include/cpn_hip.h.

* ``geometry``: bundle width, bundles, groups per bundle and items of a (C, channels per group) pair;
* ``pack_forward`` / ``pack_dgrad``: the two record layouts ``cpn_conv2d`` reads, [bundle, item, bw, 32];
* ``forward``: the grouped conv as the bundles state it -- one dense conv per bundle on the unpacked records;
* ``dilate``: the stride-2 gradient at the input's size;
* ``dgrad``: the input gradient as the identity states it -- the stride-1 conv of (the dilated) dY with the dgrad records;
* ``wgrad`` / ``bgrad``: the weight and bias gradients, and ``S`` = the sum of the absolute terms of every element;
* ``WRONG_RULES``: rules one could implement by mistake.  tests/test_grouped_conv.py shows that each of them disagrees with the right
  rule (and so with torch's own autograd) on the cases used, so a kernel that follows one of them cannot pass.

Tensors are torch float64 on the CPU, NCHW; ``cig`` = channels per group; ``rule`` selects a wrong rule (None: the right one).
"""
import torch
import torch.nn.functional as F

WRONG_RULES = ('off_group_not_zeroed', 'taps_not_flipped', 'roles_swapped_across_bundle', 'group_offset_missing',
               'padding_item_per_blob', 'dz_on_odd_grid', 'dz_sized_2hout', 'last_slab_dropped')
GROUP_WIDTHS = (4, 8, 16, 32, 64)


def geometry(c, cig):
    """-> (bw, bundles, groups per bundle, items, items with the padding item)"""
    assert cig in GROUP_WIDTHS, cig
    bw = 64 if cig == 64 else 32
    assert c >= bw and c % bw == 0, (c, cig)
    items = bw // 32 * 9
    return bw, c // bw, bw // cig, items, items + items % 2


def _pack(w, dgrad, rule):
    c, cig = int(w.shape[0]), int(w.shape[1])
    bw, bundles, gpb, items, packed = geometry(c, cig)
    out = torch.zeros(bundles, packed, bw, 32, dtype=w.dtype)
    for b in range(bundles):
        block = w[b * bw:(b + 1) * bw]  # [bw output channels of the conv, cig, 3, 3]
        if dgrad and rule == 'roles_swapped_across_bundle':  # the bundle's compact block transposed as a whole, not group by group
            block = block.transpose(0, 1).reshape(bw, cig, 3, 3)
        for item in range(items):
            chunk, tap = divmod(item, 9)
            ky, kx = divmod(tap, 3)
            sy, sx = (2 - ky, 2 - kx) if dgrad and rule != 'taps_not_flipped' else (ky, kx)
            for oc in range(bw):
                for c32 in range(32):
                    rc = 32 * chunk + c32
                    same = oc // cig == rc // cig
                    if not same and rule != 'off_group_not_zeroed':
                        continue
                    if dgrad and rule != 'roles_swapped_across_bundle':
                        out[b, item, oc, c32] = block[rc, oc % cig, sy, sx]
                    else:
                        out[b, item, oc, c32] = block[oc, rc % cig, sy, sx]
    if rule == 'padding_item_per_blob':  # one zero item behind an odd item count of the whole blob, none per bundle
        flat = out[:, :items].reshape(bundles * items, bw, 32)
        return torch.cat((flat, flat.new_zeros((bundles * items) % 2, bw, 32)))
    return out


def pack_forward(w, rule=None):
    """w [C, cig, 3, 3] -> [bundle, item = (32-channel chunk, tap), bw, 32] (+ one zero item per bundle when odd): output channel oc
    of the bundle, lane c = w[bw bundle + oc, rc mod cig, ky, kx] with rc = 32 chunk + c where oc and rc share a group, else 0."""
    return _pack(w, False, rule)


def pack_dgrad(w, rule=None):
    """... = w[bw bundle + rc, oc mod cig, 2 - ky, 2 - kx] where oc and rc share a group, else 0: the taps flipped, the channel roles
    swapped inside each group."""
    return _pack(w, True, rule)


def unpack(records):
    """records [bundle, items (+ 1), bw, 32] -> the dense weights [bundle, bw out, bw reduced, 3, 3] they state."""
    bundles, _, bw, _ = records.shape
    items = bw // 32 * 9
    return records[:, :items].reshape(bundles, bw // 32, 9, bw, 32).permute(0, 3, 1, 4, 2).reshape(bundles, bw, bw, 3, 3)


def bundle_conv(src, dense, bias=None, stride=1):
    """One dense 3x3 conv, padding 1, per bundle on its own bw channels of src."""
    bundles, bw = dense.shape[:2]
    outs = [F.conv2d(src[:, b * bw:(b + 1) * bw].double(), dense[b].double(), None, stride, 1) for b in range(bundles)]
    y = torch.cat(outs, 1)
    return y if bias is None else y + bias.double().reshape(1, -1, 1, 1)


def forward(x, w, bias=None, stride=1):
    return bundle_conv(x, unpack(pack_forward(w.double())), bias, stride)


def out_size(n, stride):
    return (n - 1) // stride + 1


def dilate(dy, size, rule=None):
    """dY [N, C, Hout, Wout] -> dZ [N, C, H, W] with dZ[..., 2 i, 2 j] = dY[..., i, j], zeros elsewhere; size = (H, W)."""
    n, c, ho, wo = dy.shape
    h, w = size
    assert (ho, wo) == (out_size(h, 2), out_size(w, 2)), (dy.shape, size)
    if rule == 'dz_sized_2hout':
        h, w = 2 * ho, 2 * wo
    dz = torch.zeros(n, c, h + 1, w + 1, dtype=dy.dtype)
    o = 1 if rule == 'dz_on_odd_grid' else 0
    dz[:, :, o:o + 2 * ho:2, o:o + 2 * wo:2] = dy
    return dz[:, :, :h, :w]


def dgrad(dy, w, stride=1, size=None, rule=None):
    """dX = the stride-1 conv of dY (stride 2: of its dilation to the input's size) with the weights the dgrad pack states."""
    dz = dy.double() if stride == 1 else dilate(dy.double(), size, rule)
    return bundle_conv(dz, unpack(pack_dgrad(w.double(), rule)))


def wgrad(x, dy, cig, stride=1, rule=None, slab_rows=None):
    """-> (dW [C, cig, 3, 3], S): dW[co, cl, ky, kx] = sum over n, y, x of dZ[n, co, y, x] X[n, cig (co // cig) + cl, y + ky - 1,
    x + kx - 1], dZ = dY at stride 1, its dilation at stride 2."""
    x = x.double()
    n, c, h, w = x.shape
    dz = dy.double() if stride == 1 else dilate(dy.double(), (h, w), rule)
    if dz.shape != x.shape:  # (a dZ of another size: its memory read with x's row pitch, as a kernel handed such a buffer would)
        dz = dz.permute(1, 0, 2, 3).reshape(c, -1)[:, :n * h * w].reshape(c, n, h, w).permute(1, 0, 2, 3)
    if rule == 'last_slab_dropped':  # the pixels of the last slab of slab_rows image rows (of the N * H rows) take no part
        rows = n * h
        keep = (rows - 1) // slab_rows * slab_rows
        dz = dz * (torch.arange(rows) < keep).reshape(n, 1, h, 1)
    groups = c // cig
    xp = F.pad(x, (1, 1, 1, 1))
    dw = torch.zeros(c, cig, 3, 3, dtype=torch.float64)
    S = torch.zeros_like(dw)
    dzg = dz.reshape(n, groups, cig, h, w)
    for ky in range(3):
        for kx in range(3):
            xs = xp[:, :, ky:ky + h, kx:kx + w].reshape(n, groups, cig, h, w)
            if rule == 'group_offset_missing':  # every group multiplies the channels of group 0
                xs = xs[:, :1].expand(n, groups, cig, h, w)
            dw[:, :, ky, kx] = torch.einsum('ngohw,ngihw->goi', dzg, xs).reshape(c, cig)
            S[:, :, ky, kx] = torch.einsum('ngohw,ngihw->goi', dzg.abs(), xs.abs()).reshape(c, cig)
    return dw, S


def bgrad(dy):
    """-> (db [C], S): the sum of dY itself over n, y, x (stride 2: NOT of its dilation -- the same number, fewer terms)."""
    dy = dy.double()
    return dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3))


def autograd64(x, w, b, dy, stride, groups):
    """torch's own fp64 autograd of F.conv2d(x, w, b, stride, 1, 1, groups) -> (y, dX, dW, db)."""
    x = x.double().clone().requires_grad_(True)
    w = w.double().clone().requires_grad_(True)
    b = None if b is None else b.double().clone().requires_grad_(True)
    y = F.conv2d(x, w, b, stride, 1, 1, groups)
    y.backward(dy.double())
    return y.detach(), x.grad, w.grad, None if b is None else b.grad
