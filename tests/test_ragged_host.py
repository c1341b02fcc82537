"""Host-side pieces of the MNIST-shaped flow (no GPU): the idx reader, the synthetic config and the reference fixture's
layout."""
import os
import struct

import numpy as np
import pytest
import torch

from lib import synthetic as syn
from lib.data import read_mnist_idx


def _write_idx(path, magic, arr, dims=None):
    dims = arr.shape if dims is None else dims
    with open(path, 'wb') as f:
        f.write(struct.pack('>I', magic))
        for d in dims:
            f.write(struct.pack('>I', d))
        f.write(arr.astype(np.uint8).tobytes())


def test_read_mnist_idx_roundtrip(tmp_path):
    rng = np.random.RandomState(0)
    imgs = rng.randint(0, 256, size=(3, 28, 28)).astype(np.uint8)
    labels = np.array([7, 0, 9], dtype=np.uint8)
    ip, lp = str(tmp_path / 'images-idx3-ubyte'), str(tmp_path / 'labels-idx1-ubyte')
    _write_idx(ip, 2051, imgs)
    _write_idx(lp, 2049, labels)
    x = read_mnist_idx(ip)
    assert x.dtype == torch.uint8 and tuple(x.shape) == (3, 1, 28, 28)
    assert np.array_equal(x[:, 0].numpy(), imgs)
    x2, y = read_mnist_idx(ip, lp)
    assert torch.equal(x, x2)
    assert y.dtype == torch.int64 and y.tolist() == [7, 0, 9]


def test_read_mnist_idx_rejects_bad_files(tmp_path):
    imgs = np.zeros((3, 28, 28), np.uint8)
    labels = np.zeros(3, np.uint8)
    bad_magic = str(tmp_path / 'bad_magic')
    _write_idx(bad_magic, 2049, imgs)                        # a label file's magic on an image file
    with pytest.raises(ValueError):
        read_mnist_idx(bad_magic)
    little = str(tmp_path / 'little_endian')
    with open(little, 'wb') as f:                            # the header written little-endian
        f.write(struct.pack('<IIII', 2051, 3, 28, 28) + imgs.tobytes())
    with pytest.raises(ValueError):
        read_mnist_idx(little)
    short = str(tmp_path / 'truncated')
    _write_idx(short, 2051, imgs[:2], dims=(3, 28, 28))      # the header promises 3 images, the file holds 2
    with pytest.raises(ValueError):
        read_mnist_idx(short)
    stub = str(tmp_path / 'stub')
    with open(stub, 'wb') as f:
        f.write(b'\x00\x00\x08')                             # shorter than a header
    with pytest.raises(ValueError):
        read_mnist_idx(stub)
    ip, lp = str(tmp_path / 'images'), str(tmp_path / 'labels')
    _write_idx(ip, 2051, imgs)
    _write_idx(lp, 2051, labels)                             # an image file's magic on a label file
    with pytest.raises(ValueError):
        read_mnist_idx(ip, lp)
    _write_idx(lp, 2049, labels[:2])                         # 2 labels for 3 images
    with pytest.raises(ValueError):
        read_mnist_idx(ip, lp)


def test_mnist_config_builds():
    from lib.configs import build_flow, imblocks
    arch = syn.MNIST
    assert syn.CONFIGS['mnist'] is arch and arch['input_size'] == (1, 28, 28) and arch['init_alpha'] == 1e-6
    assert syn.n_scales(arch['input_size'], arch['n_blocks']) == 3
    layout = syn.conv_flow_layout(arch)
    shapes = [info['shape'] for chain in layout for kind, info in chain if kind == 'imblock']
    assert shapes == [(1, 28, 28)] * 2 + [(4, 14, 14)] * 2 + [(16, 7, 7)] * 2
    small = syn.CONFIGS['mnist_small']
    m = build_flow(small, 2)
    assert len(imblocks(m)) == 3
    m.load_state_dict(syn.make_state_dict(small, 0, power_iters=2), strict=True)
    x = syn.image_batch(2, input_size=small['input_size'], seed=3)
    assert tuple(x.shape) == (2, 1, 28, 28)


def test_mnist_fixture_layout(golden_dir):
    g = np.load(os.path.join(golden_dir, 'mnist_b2.npz'))
    assert g['x'].shape == (2, 1, 28, 28) and g['x'].dtype == np.float32
    assert g['z'].shape == (2, 784) and g['logpx'].shape == (2,)
    assert int(g['nblocks']) == 3 and int(g['weight_seed']) == 0 and int(g['train']) == 0
    for i in range(3):
        for k in ('nstep', 'lowest_step', 'prot_break', 'n_power_series', 'logdet', 'z'):
            assert 'b%d_%s' % (i, k) in g.files, (i, k)
        assert g['b%d_z' % i].reshape(2, -1).shape == (2, 784)      # squeezes keep the 784 values per sample
        assert g['b%d_logdet' % i].reshape(-1).shape == (2,)
        assert np.asarray(g['b%d_n_power_series' % i]).shape == (2,)
        assert int(g['b%d_prot_break' % i]) == 0
    assert not any(k.startswith('sd:') for k in g.files)           # inputs and outputs only, no weights
    assert os.path.getsize(os.path.join(golden_dir, 'mnist_b2.npz')) < 1 << 20
