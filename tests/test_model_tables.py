"""The derived layer tables and the split forwards' buffer plans, pinned to their literal values (no device needed).

The 20 convs of the U-Net are listed once (vmatting.unet.CONVS); every other table is a view of it, and each split
forward's buffer set is a pure function of the batch shape (SplitForward.plan).  The literals below are what the
separate tables and the two ``_buffers`` held before they were derived."""

import torch

from vmatting import image_train, split3, split6, unet

NEW_CONVS = (("upconv_1", 512, 512, False), ("conv4_4", 1024, 512, True),
             ("upconv_2", 512, 256, False), ("conv3_4", 512, 256, True),
             ("upconv_3", 256, 128, False), ("conv2_3", 256, 128, True),
             ("upconv_4", 128, 64, False), ("conv1_5", 128, 1, True))

VGG_USED = ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3",
            "conv4_1", "conv4_2", "conv4_3", "conv5_1", "conv5_2")

IMAGE_LAYERS = (("conv1_1", True), ("conv1_2", True), ("conv2_1", True), ("conv2_2", True), ("conv3_1", True),
                ("conv3_2", True), ("conv3_3", True), ("conv4_1", True), ("conv4_2", True), ("conv4_3", True),
                ("conv5_1", True), ("conv5_2", True), ("upconv_1", False), ("conv4_4", True), ("upconv_2", False),
                ("conv3_4", True), ("upconv_3", False), ("conv2_3", True), ("upconv_4", False), ("conv1_5", True))

SPLIT3_LAYERS = (("conv1_1", 8, 64), ("conv1_2", 64, 64), ("conv2_1", 64, 128), ("conv2_2", 128, 128),
                 ("conv3_1", 128, 256), ("conv3_2", 256, 256), ("conv3_3", 256, 256), ("conv4_1", 256, 512),
                 ("conv4_2", 512, 512), ("conv4_3", 512, 512), ("conv5_1", 512, 512), ("conv5_2", 512, 512),
                 ("upconv_1", 512, 512), ("conv4_4", 1024, 512), ("upconv_2", 512, 256), ("conv3_4", 512, 256),
                 ("upconv_3", 256, 128), ("conv2_3", 256, 128), ("upconv_4", 128, 64), ("conv1_5", 128, 1))

SPLIT6_LAYERS = (("conv1_1", 16, 64), ("conv1_2", 64, 64), ("conv2_1", 64, 128), ("conv2_2", 128, 128),
                 ("conv3_1", 128, 256), ("conv3_2", 256, 256), ("conv3_3", 256, 256), ("conv4_1", 256, 512),
                 ("conv4_2", 512, 512), ("conv4_3", 512, 512), ("conv5_1", 512, 512), ("conv5_2", 512, 512),
                 ("upconv_1", 512, 512), ("conv4_4", 1024, 512), ("upconv_2", 512, 256), ("conv3_4", 512, 256),
                 ("upconv_3", 256, 128), ("conv2_3", 256, 128), ("upconv_4", 128, 64), ("conv1_5", 128, 8))

LEVEL = {"conv1_1": 0, "conv1_2": 0, "conv2_1": 1, "conv2_2": 1, "conv3_1": 2, "conv3_2": 2, "conv3_3": 2,
         "conv4_1": 3, "conv4_2": 3, "conv4_3": 3, "conv5_1": 4, "conv5_2": 4, "upconv_1": 3, "conv4_4": 3,
         "upconv_2": 2, "conv3_4": 2, "upconv_3": 1, "conv2_3": 1, "upconv_4": 0, "conv1_5": 0}

# buffer name -> (shape, dtype, allocated zeroed) at [n,h,w] = [2,35,61] and [1,64,96]; x3 with first_slab 32
F, H, B = torch.float32, torch.float16, torch.bfloat16
X6_2x35x61 = {
    'x': ((2, 35, 61, 96), B, True), 's11': ((2, 35, 61, 384), B, False), 'cat1': ((2, 35, 61, 768), B, False),
    'r4': ((2, 35, 61, 768), B, False), 'p1': ((2, 18, 31, 384), B, False), 's21': ((2, 18, 31, 768), B, False),
    'cat2': ((2, 18, 31, 1536), B, False), 'r3': ((2, 18, 31, 1536), B, False), 'p2': ((2, 9, 16, 768), B, False),
    's31': ((2, 9, 16, 1536), B, False), 's32': ((2, 9, 16, 1536), B, False), 'cat3': ((2, 9, 16, 3072), B, False),
    'r2': ((2, 9, 16, 3072), B, False), 'p3': ((2, 5, 8, 1536), B, False), 's41': ((2, 5, 8, 3072), B, False),
    's42': ((2, 5, 8, 3072), B, False), 'cat4': ((2, 5, 8, 6144), B, False), 'r1': ((2, 5, 8, 3072), B, False),
    'p4': ((2, 3, 4, 3072), B, False), 's51': ((2, 3, 4, 3072), B, False), 'f0': ((2, 35, 61, 128), F, False),
    'f1': ((2, 18, 31, 256), F, False), 'f2': ((2, 9, 16, 512), F, False), 'f3': ((2, 5, 8, 512), F, False),
    'f4': ((2, 3, 4, 512), F, False), 'rr0': ((2, 35, 61, 128), F, False), 'rr1': ((2, 18, 31, 256), F, False),
    'rr2': ((2, 9, 16, 512), F, False), 'rr3': ((2, 5, 8, 512), F, False), 'lg0': ((2, 35, 61, 1), F, False),
    'lg1': ((2, 35, 61, 1), F, False), 'lg2': ((2, 35, 61, 1), F, False), 'zero': ((2, 35, 61, 1), F, True),
    'out': ((2, 35, 61, 1), F, False)}

X6_1x64x96 = {
    'x': ((1, 64, 96, 96), B, True), 's11': ((1, 64, 96, 384), B, False), 'cat1': ((1, 64, 96, 768), B, False),
    'r4': ((1, 64, 96, 768), B, False), 'p1': ((1, 32, 48, 384), B, False), 's21': ((1, 32, 48, 768), B, False),
    'cat2': ((1, 32, 48, 1536), B, False), 'r3': ((1, 32, 48, 1536), B, False), 'p2': ((1, 16, 24, 768), B, False),
    's31': ((1, 16, 24, 1536), B, False), 's32': ((1, 16, 24, 1536), B, False),
    'cat3': ((1, 16, 24, 3072), B, False), 'r2': ((1, 16, 24, 3072), B, False), 'p3': ((1, 8, 12, 1536), B, False),
    's41': ((1, 8, 12, 3072), B, False), 's42': ((1, 8, 12, 3072), B, False), 'cat4': ((1, 8, 12, 6144), B, False),
    'r1': ((1, 8, 12, 3072), B, False), 'p4': ((1, 4, 6, 3072), B, False), 's51': ((1, 4, 6, 3072), B, False),
    'f0': ((1, 64, 96, 128), F, False), 'f1': ((1, 32, 48, 256), F, False), 'f2': ((1, 16, 24, 512), F, False),
    'f3': ((1, 8, 12, 512), F, False), 'f4': ((1, 4, 6, 512), F, False), 'rr0': ((1, 64, 96, 128), F, False),
    'rr1': ((1, 32, 48, 256), F, False), 'rr2': ((1, 16, 24, 512), F, False), 'rr3': ((1, 8, 12, 512), F, False),
    'lg0': ((1, 64, 96, 1), F, False), 'lg1': ((1, 64, 96, 1), F, False), 'lg2': ((1, 64, 96, 1), F, False),
    'zero': ((1, 64, 96, 1), F, True), 'out': ((1, 64, 96, 1), F, False)}

X3_2x35x61 = {
    'x': ((2, 35, 61, 64), H, True), 's11': ((2, 35, 61, 128), H, False), 'cat1': ((2, 35, 61, 256), H, False),
    'r4': ((2, 35, 61, 256), H, False), 'p1': ((2, 18, 31, 128), H, False), 's21': ((2, 18, 31, 256), H, False),
    'cat2': ((2, 18, 31, 512), H, False), 'r3': ((2, 18, 31, 512), H, False), 'p2': ((2, 9, 16, 256), H, False),
    's31': ((2, 9, 16, 512), H, False), 's32': ((2, 9, 16, 512), H, False), 'cat3': ((2, 9, 16, 1024), H, False),
    'r2': ((2, 9, 16, 1024), H, False), 'p3': ((2, 5, 8, 512), H, False), 's41': ((2, 5, 8, 1024), H, False),
    's42': ((2, 5, 8, 1024), H, False), 'cat4': ((2, 5, 8, 2048), H, False), 'r1': ((2, 5, 8, 1024), H, False),
    'p4': ((2, 3, 4, 1024), H, False), 's51': ((2, 3, 4, 1024), H, False), 'c44s': ((2, 5, 8, 1024), H, False),
    'c34s': ((2, 9, 16, 512), H, False), 'c23s': ((2, 18, 31, 256), H, False), 'f0': ((2, 35, 61, 128), F, False),
    'f1': ((2, 18, 31, 256), F, False), 'f2': ((2, 9, 16, 512), F, False), 'f3': ((2, 5, 8, 512), F, False),
    'f4': ((2, 3, 4, 512), F, False), 'lg0': ((2, 35, 61, 1), F, False), 'out': ((2, 35, 61, 1), F, False)}

X3_1x64x96 = {
    'x': ((1, 64, 96, 64), H, True), 's11': ((1, 64, 96, 128), H, False), 'cat1': ((1, 64, 96, 256), H, False),
    'r4': ((1, 64, 96, 256), H, False), 'p1': ((1, 32, 48, 128), H, False), 's21': ((1, 32, 48, 256), H, False),
    'cat2': ((1, 32, 48, 512), H, False), 'r3': ((1, 32, 48, 512), H, False), 'p2': ((1, 16, 24, 256), H, False),
    's31': ((1, 16, 24, 512), H, False), 's32': ((1, 16, 24, 512), H, False), 'cat3': ((1, 16, 24, 1024), H, False),
    'r2': ((1, 16, 24, 1024), H, False), 'p3': ((1, 8, 12, 512), H, False), 's41': ((1, 8, 12, 1024), H, False),
    's42': ((1, 8, 12, 1024), H, False), 'cat4': ((1, 8, 12, 2048), H, False), 'r1': ((1, 8, 12, 1024), H, False),
    'p4': ((1, 4, 6, 1024), H, False), 's51': ((1, 4, 6, 1024), H, False), 'c44s': ((1, 8, 12, 1024), H, False),
    'c34s': ((1, 16, 24, 512), H, False), 'c23s': ((1, 32, 48, 256), H, False), 'f0': ((1, 64, 96, 128), F, False),
    'f1': ((1, 32, 48, 256), F, False), 'f2': ((1, 16, 24, 512), F, False), 'f3': ((1, 8, 12, 512), F, False),
    'f4': ((1, 4, 6, 512), F, False), 'lg0': ((1, 64, 96, 1), F, False), 'out': ((1, 64, 96, 1), F, False)}


def test_derived_tables_equal_their_literals():
    assert unet.NEW_CONVS == NEW_CONVS
    assert unet.VGG_USED == VGG_USED
    assert image_train.LAYERS == IMAGE_LAYERS
    assert split3.LAYERS == SPLIT3_LAYERS
    assert split6.LAYERS == SPLIT6_LAYERS
    assert unet.LEVEL == LEVEL
    assert [row[0] for row in unet.CONVS] == [name for name, _ in IMAGE_LAYERS]  # TF build order
    assert unet.CONVS[0][2] is None  # conv1_1's cin is the model's IN_CH


def test_one_levels_function():
    from vmatting import unet_simple
    assert unet_simple._levels is unet._levels
    assert unet._levels(35, 61) == [(35, 61), (18, 31), (9, 16), (5, 8), (3, 4)]


def _plan(cls, shape, **attrs):
    fwd = object.__new__(cls)  # the plan reads the class's constants only: no model, no device
    for k, v in attrs.items():
        setattr(fwd, k, v)
    return fwd.plan(*shape)


def test_split6_buffer_plan():
    assert _plan(split6.Split6Forward, (2, 35, 61)) == X6_2x35x61
    assert _plan(split6.Split6Forward, (1, 64, 96)) == X6_1x64x96


def test_split3_buffer_plan():
    assert split3.Split3Forward.first_slab == 32
    assert _plan(split3.Split3Forward, (2, 35, 61)) == X3_2x35x61
    assert _plan(split3.Split3Forward, (1, 64, 96)) == X3_1x64x96
    # first_slab 8: [l, h, h] + a zero 4th slab in one 32-channel granule
    assert _plan(split3.Split3Forward, (2, 35, 61), first_slab=8) == dict(X3_2x35x61, x=((2, 35, 61, 32), H, True))
    assert _plan(split3.Split3Forward, (1, 64, 96), first_slab=8) == dict(X3_1x64x96, x=((1, 64, 96, 32), H, True))
