"""The sub-pixel forward of the deep conv3x3(nearest_x2(x)) layers on the SIMT emulator (tests/up_deep_checks.py): indexing, placement,
the ordered split and its finishing pass, bounds - before a GPU minute is spent.  The hardware twin is tests/test_up_deep_gpu.py."""
import pytest
import torch

import up_deep_checks as ud

DEV = torch.device("cpu")


@pytest.mark.parametrize("split", [1, 2, 3])
@pytest.mark.parametrize("tile", ud.TILES)
def test_every_tile_and_split(emu_lib, tile, split):
    """Cin 512, source 4 x 4, N = 2, Cout 40 (ragged N tile, % 4 == 0), bias + LeakyReLU + wscale"""
    ud.check_entry(DEV, 2, 4, 4, 512, 40, True, tile, split)


@pytest.mark.parametrize("tile,split", [(4, 1), (9, 2), (0, 3), (-1, 0)])
def test_odd_extents(emu_lib, tile, split):
    """source 5 x 3, N = 1: a border in every class, rows that wrap inside a pixel tile; no epilogue"""
    ud.check_entry(DEV, 1, 5, 3, 512, 40, False, tile, split)


@pytest.mark.parametrize("tile,split", [(9, 1), (0, 2), (1, 3), (2, 2), (4, 2)])
def test_several_channel_tiles(emu_lib, tile, split):
    """Cout 160: more than one N tile in every tile shape"""
    ud.check_entry(DEV, 1, 5, 3, 512, 160, tile in (9, 1), tile, split)


def test_split_and_unsplit_agree(emu_lib):
    """the order of the sum changes with the split, the value does not beyond fp32 rounding"""
    a = ud.run_entry(DEV, 2, 4, 4, 512, 40, True, 4, 1)[0]
    b = ud.run_entry(DEV, 2, 4, 4, 512, 40, True, 4, 3)[0]
    ud.assert_close('split 3 vs unsplit', b, a, 2e-6)


def test_rejections(emu_lib):
    ud.check_rejections(DEV)


def test_backward_undisturbed(emu_lib):
    ud.check_backward_undisturbed(DEV)


def test_selection(emu_lib):
    ud.check_selection(DEV)


def test_layout_cache_path(emu_lib):
    ud.check_cache_path(DEV)
