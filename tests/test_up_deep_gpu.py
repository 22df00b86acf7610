"""The sub-pixel forward of the deep conv3x3(nearest_x2(x)) layers on hardware (tests/up_deep_checks.py; emulator twin:
tests/test_up_deep_emu.py): every tile shape of the group dispatch x split 1 / 2 / 3, odd extents, several channel tiles, the
selection in ops.conv2d and the two production shapes' plans."""
import pytest
import torch

import up_deep_checks as ud

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("split", [1, 2, 3])
@pytest.mark.parametrize("tile", ud.TILES)
@pytest.mark.parametrize("epilogue", [True, False])
def test_every_tile_and_split(hip_lib, epilogue, tile, split):
    ud.check_entry(DEV, 2, 4, 4, 512, 40, epilogue, tile, split)


@pytest.mark.parametrize("split", [0, 1, 2, 3])
@pytest.mark.parametrize("tile", (-1,) + ud.TILES)
def test_odd_extents(hip_lib, tile, split):
    ud.check_entry(DEV, 1, 5, 3, 512, 40, False, tile, split)


@pytest.mark.parametrize("split", [1, 2, 3])
@pytest.mark.parametrize("tile", ud.TILES)
def test_several_channel_tiles(hip_lib, tile, split):
    ud.check_entry(DEV, 1, 5, 3, 512, 160, True, tile, split)


def test_split_and_unsplit_agree(hip_lib):
    a = ud.run_entry(DEV, 2, 4, 4, 512, 40, True, 4, 1)[0]
    b = ud.run_entry(DEV, 2, 4, 4, 512, 40, True, 4, 3)[0]
    ud.assert_close('split 3 vs unsplit', b, a, 2e-6)


def test_production_shapes_plan_and_run(hip_lib):
    """the two deep layers of the flagship workload (source 16 x 16 Cin 1024 -> 512, source 32 x 32 Cin 1024 -> 256, B = 2): the plan
    fills the chip (at least 256 workgroups) and the planned launch meets the fp64 bar"""
    ops, _ = ud.pkg()
    for h, cout in ((16, 512), (32, 256)):
        tile, nsplit, need = ops.up_subpixel_plan(2, h, h, 1024, cout)
        bm, bn = {0: (128, 128), 1: (128, 64), 2: (128, 32), 4: (64, 64), 9: (64, 128)}[tile]
        assert 4 * (-(-2 * h * h // bm)) * (-(-cout // bn)) * nsplit >= 256, (tile, nsplit)
        assert need == (4 * nsplit * 2 * h * h * cout if nsplit > 1 else 0)
        ud.check_entry(DEV, 2, h, h, 1024, cout, True, -1, 0)


def test_rejections(hip_lib):
    ud.check_rejections(DEV)


def test_backward_undisturbed(hip_lib):
    ud.check_backward_undisturbed(DEV)


def test_selection(hip_lib):
    ud.check_selection(DEV)


def test_layout_cache_path(hip_lib):
    ud.check_cache_path(DEV)
