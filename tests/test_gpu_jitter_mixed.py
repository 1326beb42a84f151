"""ops.color_jitter_mixed (oibl_color_jitter_u8_mixed) on the device: every image of a packed batch of mixed sizes is
bit-equal to the uniform kernel on that image alone (ops.color_jitter, which tests/test_gpu_color_jitter.py holds to
PIL), out of place and in place, in any batch order, run after run; the padding between the images and an image whose
table row is inconsistent are never touched.  Every comparison is bit equality."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import color_jitter_ref as ref
from openibl_amd import jpeg, lib, ops

pytestmark = pytest.mark.gpu

B, C, S, H, X = ref.BRIGHTNESS, ref.CONTRAST, ref.SATURATION, ref.HUE, ref.SKIP
# 8 x 8; H W 3 = 3 mod 4; exactly one chunk of 4096 pixels; one chunk and a tail; five parts; 48 x 64; 1 pixel; 1 mod 4
SIZES = ((8, 8), (37, 53), (64, 64), (64, 65), (120, 160), (48, 64), (1, 1), (5, 7), (64, 64))
ORDERS = ((C, B, S, H), (B, C, H, S), (H, S, C, B), (S, H, B, C), (B, S, H, X), (X, X, X, X), (H, C, X, B),
          (S, X, C, X), (C, H, S, B))
FILL = 0xA5


def records(n, seed=11):
    rng = np.random.default_rng(seed)
    orders = [ORDERS[i % len(ORDERS)] for i in range(n)]
    return ref.pack_records(orders, rng.uniform(0.3, 1.7, (n, 3)), [ref.hue_byte(v) for v in rng.uniform(-0.5, 0.5, n)])


def image(i, h, w):
    """Image i of the batch: the same content wherever it stands."""
    img = np.random.default_rng(500 + i).integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[: max(h // 4, 1)] //= 8
    return img


def pack(order, sizes=SIZES):
    """(packed uint8 with the padding filled, offsets, padding mask) of the images `order` of `sizes`."""
    sz = [sizes[i] for i in order]
    geom, totals = jpeg.mixed_layout(sz)
    offs = jpeg.geom_pixel_offsets(geom).tolist()
    packed = np.full(totals[2], FILL, np.uint8)
    pad = np.ones(totals[2], bool)
    for i, (h, w), o in zip(order, sz, offs):
        packed[o:o + 3 * h * w] = image(i, h, w).reshape(-1)
        pad[o:o + 3 * h * w] = False
    return packed, offs, pad


@pytest.fixture(scope="module")
def alone(dev):
    """Image i through the UNIFORM kernel on its own, with record i: the reference of every test here, computed once."""
    rec = records(len(SIZES))
    out = []
    for i, (h, w) in enumerate(SIZES):
        x = torch.from_numpy(image(i, h, w))[None].to(dev)
        out.append(ops.color_jitter(x, torch.from_numpy(rec[i:i + 1]).to(dev), out="uint8")[0].cpu().numpy())
    return rec, out


def images_of(buf, order, offs):
    return [buf[o:o + 3 * SIZES[i][0] * SIZES[i][1]].reshape(*SIZES[i], 3) for i, o in zip(order, offs)]


@pytest.mark.parametrize("order", [tuple(range(9)), tuple(reversed(range(9))), (4, 1, 6, 3)],
                         ids=["forward", "reversed", "four"])
def test_every_image_is_the_uniform_kernel_on_it_alone(dev, alone, order):
    rec, want = alone
    order = list(order)
    sizes = [SIZES[i] for i in order]
    packed, offs, pad = pack(order)
    x = torch.from_numpy(packed).to(dev)
    params = torch.from_numpy(rec[order]).to(dev)
    assert pad.sum() > 0 and any((3 * h * w) % 4 for h, w in sizes)
    # out of place: the input is untouched, the output's images are the uniform kernel's
    out = torch.full_like(x, 0x3C)
    got = ops.color_jitter_mixed(x, sizes, params, out=out)
    assert got is out and np.array_equal(x.cpu().numpy(), packed)
    res = out.cpu().numpy()
    assert (res[pad] == 0x3C).all()                               # the padding of the output is not written either
    for k, (i, img) in enumerate(zip(order, images_of(res, order, offs))):
        assert np.array_equal(img, want[i]), (order, k, SIZES[i])
    # a fresh buffer when none is given
    fresh = ops.color_jitter_mixed(x, sizes, params)
    assert fresh.data_ptr() != x.data_ptr() and fresh.shape == x.shape
    for i, img in zip(order, images_of(fresh.cpu().numpy(), order, offs)):
        assert np.array_equal(img, want[i])
    # in place: the same bytes, and the pattern between the images is still there
    y = x.clone()
    assert ops.color_jitter_mixed(y, sizes, params, out=y) is y
    inp = y.cpu().numpy()
    assert (inp[pad] == FILL).all()
    assert np.array_equal(inp[~pad], res[~pad])
    # again: the same bits
    z = x.clone()
    ops.color_jitter_mixed(z, sizes, params, out=z)
    assert torch.equal(z, y)


def test_without_records_the_images_are_copied_and_in_place_nothing_happens(dev):
    order = list(range(len(SIZES)))
    packed, offs, pad = pack(order)
    x = torch.from_numpy(packed).to(dev)
    out = torch.full_like(x, 0x3C)
    ops.color_jitter_mixed(x, SIZES, None, out=out)
    res = out.cpu().numpy()
    assert np.array_equal(res[~pad], packed[~pad]) and (res[pad] == 0x3C).all()
    y = x.clone()
    assert ops.color_jitter_mixed(y, SIZES, None, out=y) is y and torch.equal(y, x)


def test_a_large_image_whose_chunks_grow_sits_between_small_ones(dev):
    """1100 x 4000: 538 parts of 8192 pixels (more than 1024 chunks of 4096), between a 37 x 53 and an 8 x 8 image
    whose workgroups beyond their one part leave at once."""
    sizes = [(37, 53), (1100, 4000), (8, 8)]
    rec = records(3, seed=5)
    rec[1, :4] = (S, C, H, B)                                      # contrast behind a prefix: 538 partial sums
    g = torch.Generator().manual_seed(9)
    imgs = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g) for h, w in sizes]
    geom, totals = jpeg.mixed_layout(sizes)
    offs = jpeg.geom_pixel_offsets(geom).tolist()
    x = torch.full((totals[2],), FILL, dtype=torch.uint8)
    for img, o in zip(imgs, offs):
        x[o:o + img.numel()] = img.reshape(-1)
    x = x.to(dev)
    params = torch.from_numpy(rec).to(dev)
    ops.color_jitter_mixed(x, sizes, params, out=x)
    for n, (img, o) in enumerate(zip(imgs, offs)):
        want = ops.color_jitter(img[None].to(dev), params[n:n + 1], out="uint8")[0]
        assert torch.equal(x[o:o + img.numel()].view_as(want), want), sizes[n]
    pad = torch.ones(totals[2], dtype=torch.bool)
    for img, o in zip(imgs, offs):
        pad[o:o + img.numel()] = False
    assert bool((x.cpu()[pad] == FILL).all())


def test_an_inconsistent_row_leaves_its_image_alone_and_hurts_nobody(dev, alone):
    """A validation test, bounded by construction: the row's offset lies beyond packed_bytes, the kernel refuses the
    row before it forms an address.  The image's output bytes keep their pattern; every other image is unchanged."""
    rec, want = alone
    order = list(range(len(SIZES)))
    packed, offs, pad = pack(order)
    sizes = np.ascontiguousarray(np.asarray(SIZES, np.int32))
    geom, totals = jpeg.mixed_layout(sizes)
    h = lib.load()
    sp = sizes.ctypes.data_as(ctypes.c_void_p)
    x = torch.from_numpy(packed).to(dev)
    params = torch.from_numpy(rec).to(dev)
    ws = ops.workspace(h.oibl_color_jitter_u8_mixed_workspace_bytes(sp, len(SIZES)), dev, slot="color_jitter")
    for bad, entry, value in ((4, 4, totals[2]), (1, 5, 1), (2, 0, -3), (0, 4, totals[2] - 100)):
        table = geom.copy()
        table[bad, entry] = value
        out = torch.full_like(x, 0x3C)
        table_dev = torch.from_numpy(table).to(dev)
        rc = h.oibl_color_jitter_u8_mixed(x.data_ptr(), x.numel(), table_dev.data_ptr(), sp,
                                          len(SIZES), params.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                          torch.cuda.current_stream(dev).cuda_stream)
        lib.check(rc, "color_jitter_u8_mixed")
        res = out.cpu().numpy()
        hh, ww = SIZES[bad]
        assert (res[offs[bad]:offs[bad] + 3 * hh * ww] == 0x3C).all(), (bad, entry, value)
        assert (res[pad] == 0x3C).all()
        for i, img in enumerate(images_of(res, order, offs)):
            if i != bad:
                assert np.array_equal(img, want[i]), (bad, entry, value, i)
    torch.cuda.synchronize(dev)
