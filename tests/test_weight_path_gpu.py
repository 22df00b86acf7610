"""The weight path - K-major layouts, weight-gradient finalisation, spectral-norm backward and power iteration - on a real MI355X
against fp64 PyTorch on the CPU (tests/weight_path_checks.py): the checks of tests/test_weight_path_emu.py, same shapes, same bounds."""
import pytest
import torch

import weight_path_checks as wc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("cout", wc.COUTS)
@pytest.mark.parametrize("geom", wc.GEOMS)
def test_layouts(hip_lib, geom, cout):
    for cin in wc.CINS:
        for cpad in wc.CPADS:
            wc.check_layouts(DEV, geom[0], geom[1], cout, cin, cpad)


@pytest.mark.parametrize("geom", wc.GEOMS)
def test_prep_weight_modes(hip_lib, geom):
    for cout in wc.COUTS:
        for cin in wc.CINS:
            wc.check_prep_weight_modes(DEV, geom[0], geom[1], cout, cin)


@pytest.mark.parametrize("cout", wc.COUTS)
@pytest.mark.parametrize("geom", wc.GEOMS)
def test_finalize_geometry(hip_lib, geom, cout):
    for cin in wc.CINS:
        for cpad in wc.CPADS:
            wc.check_finalize_geometry(DEV, geom[0], geom[1], cout, cin, cpad)


def test_finalize_tap_subset(hip_lib):
    wc.check_finalize_tap_subset(DEV)


def test_finalize_shared_sink(hip_lib):
    wc.check_finalize_shared_sink(DEV)


def test_finalize_five_jobs(hip_lib):
    wc.check_finalize_five_jobs(DEV)


def test_finalize_long_dot(hip_lib):
    wc.check_finalize_long_dot(DEV)


def test_finalize_layout_cache_words_and_round_trip(hip_lib):
    wc.check_finalize_layout_cache(DEV)


def test_finalize_bad_args(hip_lib):
    assert wc.check_finalize_bad_args(DEV) == 8


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("shape", wc.SN_BWD_SHAPES)
def test_sn_backward(hip_lib, shape, accumulate):
    wc.check_sn_backward(DEV, shape[0], shape[1], accumulate)


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", wc.SN_BWD_OFFSETS)
def test_sn_backward_unaligned(hip_lib, case, accumulate):
    wc.check_sn_backward(DEV, case[0], case[1], accumulate, off=case[2])


def test_sn_backward_agrees_with_finalize(hip_lib):
    wc.check_sn_backward_vs_finalize(DEV)


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("shape", wc.POWER_SHAPES)
def test_power_iteration(hip_lib, shape, training):
    wc.check_power_iteration(DEV, shape[0], shape[1], training)


def test_power_iteration_batched(hip_lib):
    wc.check_power_iteration_batched(DEV)
