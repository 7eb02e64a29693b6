"""Every conv kernel instantiation at its tile edges, by name (the case table: tests/conv_tiles.py).

One case per reachable conv_igemm_kernel<TH, BN, WM, WN, MODE> of the bf16 and the e4m3 unit, and one per second epilogue on
a big and a small tile of each mode.  Each case first asks the library once more which kernel it runs
(cpn_conv2d_kernel_info: the selection step of the launch itself) and fails if that is not the key's; then it runs through
test_gpu_kernels.run_conv / run_conv_fp8 / the bridge test and is held to the bounds of tests/conv_bounds.py, unchanged:
bf16 outputs RNE of the accumulation-noise window of the fp64 conv of the same operands, e4m3 outputs the code window, fp32
outputs noise + 4 ulp; guard bands untouched, padded channels zero.

A failure names the instantiation and says whether the worst element lies in an edge row tile, an edge column tile or the
last channel block (conv_tiles.locate, from the failing index, TH, BN and 32).
"""
import pytest
import torch

import conv_bounds as cb
import conv_tiles as ct
import test_gpu_conv_bridge as tb
import test_gpu_kernels as tk

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


@pytest.mark.parametrize('key', list(ct.TABLE))
def test_conv_instantiation_at_its_tile_edges(dev, key, monkeypatch):
    unit, mode, th, bn, _ = ct.parse_key(key)
    for name, value in ct.ENV.get(key, {}).items():
        monkeypatch.setenv(name, value)
    info = ct.query(key)
    assert info[:3] == (mode, th, bn), f'{key}: the library runs {ct.info_key(unit, info)} here'
    cfg = ct.TABLE[key]
    if 'bridge' in cfg:  # MODE_BR: its own test (bit-identical to the two launches it replaces, both within the bound)
        tb.test_conv_bridge_kernel(dev, cfg['bridge'])
        return
    try:
        if unit == 'e4m3':
            ratio = tk.run_conv_fp8(dev, key, **cfg)
        else:
            got, chk, _ = tk.run_conv(dev, **cfg)
            try:
                ratio = chk(key, got)
            except cb.BoundError as e:
                e.got, e.lo, e.hi, e.ref = got, chk.lo, chk.hi, chk.ref
                raise
    except cb.BoundError as e:
        index, _ = ct.worst(e.got, e.lo, e.hi, e.ref)
        raise cb.BoundError(f'{ct.locate(key, info, index, tuple(e.got.shape))}\n{e}') from None
    if unit != 'e4m3':  # (run_conv_fp8 prints its own)
        print(f'{key}: max |got - ref| / bound = {ratio:.3g}')
