"""CPU logic tests of the optimiser, loss-scale, cross-replica BatchNorm, max-pool and table-helper entry points: the HIP kernel
sources executed by the SIMT emulator against fp64 PyTorch (tests/small_op_checks.py).  tests/test_small_ops_gpu.py runs the same
checks on the hardware."""
import pytest
import torch

import small_op_checks as sc

DEV = torch.device("cpu")


@pytest.mark.parametrize("gscale", sc.ADAM_GSCALES)
@pytest.mark.parametrize("betas", sc.ADAM_BETAS)
def test_adam_against_fp64(emu_lib, betas, gscale):
    sc.check_adam_fp64(DEV, betas, gscale)


def test_adam_step_in_ranges(emu_lib):
    sc.check_adam_ranges(DEV)


def test_amp_adam(emu_lib):
    sc.check_amp_adam(DEV)


@pytest.mark.parametrize("n", sc.AMP_CHECK_SIZES)
def test_amp_check(emu_lib, n):
    sc.check_amp_check(DEV, n)


def test_amp_update(emu_lib):
    sc.check_amp_update(DEV)


@pytest.mark.parametrize("act", ['none', 'lrelu'])
@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("shape", sc.SYNC_BN_SHAPES)
def test_sync_bn(emu_lib, shape, world, act):
    sc.check_sync_bn(DEV, shape[0], shape[1], world, act)


def test_sync_bn_cancellation(emu_lib):
    sc.check_sync_bn_cancellation(DEV)


@pytest.mark.parametrize("shape", sc.MAXPOOL_SHAPES)
def test_maxpool2(emu_lib, shape):
    sc.check_maxpool2(DEV, shape)


@pytest.mark.parametrize("count", [4, 1028, 70000, 1027, 70001])      # the last two end in the scalar tail of a block
@pytest.mark.parametrize("nsrc", [1, 2, 3, 4])
def test_sum_terms_one_job(emu_lib, nsrc, count):
    sc.check_sum_terms(DEV, [nsrc], [count])


def test_sum_terms_eight_jobs(emu_lib):
    sc.check_sum_terms(DEV, [1, 2, 3, 4, 4, 3, 2, 1], [4, 1028, 70000, 4, 1028, 70000, 1028, 4])
    sc.check_sum_terms(DEV, [4, 3, 2, 1, 1, 2, 3, 4], [70001, 1027, 5, 1028, 70001, 1027, 6, 7])


@pytest.mark.parametrize("sizes", [(1,), (4095,), (4096,), (4097,), (20000,), (1, 4095, 4096, 4097, 20000)])
def test_gather_add(emu_lib, sizes):
    sc.check_gather_add(DEV, sizes)


def test_upload_i64(emu_lib):
    per_launch = sc.upload_words_per_launch()
    for n in (1, 7, 64, per_launch, per_launch + 1, 2 * per_launch + 104):
        sc.check_upload_i64(DEV, n)


@pytest.mark.parametrize("shape", [(1000, 7), (300, 260)])
def test_two_launch_reductions(emu_lib, shape):
    sc.check_two_launch_reductions(DEV, shape[0], shape[1])


@pytest.mark.parametrize("total", sc.ACT_SIZES)
def test_act_fwd(emu_lib, total):
    sc.check_act_fwd(DEV, total)


def test_bias_act(emu_lib):
    assert sc.check_bias_act(DEV) == len(sc.BIAS_ACT_TOTALS) * len(sc.BIAS_ACT_CHANNELS) * len(sc.ACT_CODES) == 54


def test_blend_bwd(emu_lib):
    assert sc.check_blend_bwd(DEV) == 8
