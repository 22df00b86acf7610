"""Every instantiated tile of the fp32 GEMM kernels on the SIMT emulator (tests/tile_checks.py)."""
import json
import os

import pytest
import torch

import op_checks as oc
import tile_checks as tc

CPU = torch.device('cpu')
# every id the table holds today, pinned here so that the walk is one test per id and a row that goes missing shows
TABLE_IDS = tc.FWD_TILES + tuple(v for v, _ in tc.EXPERIMENTAL_FWD_TILES) + tc.REORDERED_FWD_TILES


@pytest.mark.parametrize('tile', tc.FWD_TILES)
def test_forward_tile(tile):
    tc.check_forward_tiles(CPU, tiles=(tile,), geoms=tc.GEOMS)


def test_per_sample_tiles():
    tc.check_per_sample(CPU)


@pytest.mark.parametrize('tile', tc.WGRAD_TILES)
def test_wgrad_tile(tile):
    tc.check_wgrad_tiles(CPU, tiles=(tile,))


@pytest.mark.parametrize('variant,base', tc.EXPERIMENTAL_FWD_TILES)
def test_prefetch_two_variant(variant, base):
    """force_tile-only prefetch-distance-2 kernels: against F.conv2d and bit-equal to the plan's tile of the same shape, over
    chunk counts 1 ... 11 per K split (odd and even: the loop runs two chunks per trip)"""
    tc.check_forward_tiles(CPU, tiles=(variant,), geoms=tc.GEOMS)
    tc.check_variant_equals_plan_tile(CPU, variant, base)


@pytest.mark.parametrize('tile', tc.REORDERED_FWD_TILES)
def test_lds_direct_variant(tile):
    """loads straight into LDS, three buffers, whole trips of three chunks (chunk counts 1 ... 11 per split: every remainder)"""
    tc.check_forward_tiles(CPU, tiles=(tile,), geoms=tc.GEOMS)


def test_table_ids_are_the_pinned_ones():
    assert sorted(tc.tile_table()) == sorted(TABLE_IDS)


def test_tile_labels_are_the_recorded_ones():
    """tools/trace_by_grid.py, tools/launch_report.py and the CSVs under profiles/ match on these strings"""
    from importlib import import_module
    oc.pkg()
    profile = import_module('few-shot-vid2vid_amd.profile')
    assert {t: profile.tile_name(t) for t in TABLE_IDS} == {
        0: '128x128', 1: '128x64', 2: '128x32', 4: '64x64', 9: '64x128', 10: '64x128pf2', 11: '128x128pf2', 12: '128x64pf2',
        13: '64x128pf2af', 14: '128x128pf2af', 15: '128x64pf2af', 16: '128x128af', 17: '64x64af', 18: '128x32af', 20: '64x64pf2af',
        21: '64x128lds', 22: '128x64lds', 27: '64x64lds'}


@pytest.mark.parametrize('tile', TABLE_IDS)
def test_table_walk(tile):
    """the id through all four dispatchers (plain, folded up-sampling, grouped, scalar gather)"""
    tc.check_table_walk(CPU, ids=(tile,))


def test_table_walk_refuses_what_is_no_row():
    tc.check_table_refusals(CPU)


def _plan_fixture():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_plan.json')) as f:
        return json.load(f)


def test_plans_match_the_recorded_ones(monkeypatch):
    """fsv_conv_plan and fsv_conv_group_plan decide what they decided when tests/golden/conv_plan.json was recorded
    (tools/conv_plan_golden.py): the step's shapes, threshold and ragged sizes, forced tiles and splits, groups of 2 / 5 / 17"""
    for name in [k for k in os.environ if k.startswith('FSV_')]:
        monkeypatch.delenv(name)
    conv = oc.pkg()[1]
    fx = _plan_fixture()
    assert len(fx['plan']) >= 300 and {len(g) for g, _ in fx['groups']} == {2, 5, 17}
    bad = [(row, conv.planned(*row[:6])) for row in fx['plan'] if conv.planned(*row[:6]) != tuple(row[6:])]
    assert not bad, bad[:10]
    bad = [(g, t, conv.group_planned(g)) for g, t in fx['groups'] if conv.group_planned(g) != t]
    assert not bad, bad[:10]


def test_deterministic_mode_plans_no_split(monkeypatch):
    """FSV_DETERMINISTIC=1: every row of the fixture that does not force a split plans one pass over K"""
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    conv = oc.pkg()[1]
    rows = [row for row in _plan_fixture()['plan'] if row[5] == 0]
    assert len(rows) >= 300
    bad = [row for row in rows if conv.planned(*row[:6])[1] != 1]
    assert not bad, bad[:10]
