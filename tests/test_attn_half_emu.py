"""The streaming few-shot attention on the f16 matrix cores (few-shot-vid2vid_amd/csrc/attention_h.hip, ops.attention_fused_half,
FSV_ATTN_FUSED_HALF, InferenceSession(fused_attention='half')) on the emulator: the prep launch bit for bit, the operator against
float64 at the derived bound and at the output bar, the low parts of the split, key ranges, rescaling, determinism, the untouched
default path, the bounds and the kept session.  The real size is tools/attn_half.py's, on hardware."""
import pytest
import torch

import attn_half_checks as ah

DEV = torch.device('cpu')


@pytest.fixture(autouse=True)
def _fixed_order(monkeypatch):
    monkeypatch.setenv('FSV_DETERMINISTIC', '1')
    for k in (ah.SWITCH, ah.af.SWITCH, ah.ab.SWITCH):
        monkeypatch.delenv(k, raising=False)


def test_half_prep_is_bit_exact_emu(emu_lib):
    ah.check_prep(DEV)


@pytest.mark.parametrize('second', ['announced', 'unannounced', 'absent'])
@pytest.mark.parametrize('case', ['small', 'c24', 'ragged', 'prod'])
def test_half_attention_against_float64_emu(emu_lib, case, second):
    ah.check_operator(DEV, case, second)


def test_low_parts_of_the_split_emu(emu_lib):
    ah.check_offset(DEV)


def test_half_key_ranges_and_finishing_pass_emu(emu_lib):
    ah.check_splits(DEV)


@pytest.mark.parametrize('placement', ['first', 'last'])
def test_half_online_softmax_rescaling_emu(emu_lib, placement):
    ah.check_rescale(DEV, placement)


def test_half_same_bits_on_every_run_emu(emu_lib):
    ah.check_determinism(DEV)


def test_half_switch_leaves_the_default_path_emu(emu_lib):
    ah.check_default_path(DEV)


def test_half_entry_point_bounds_emu(emu_lib):
    ah.check_bounds(DEV)


@pytest.mark.parametrize('name', ['mul', 'concat'])
def test_half_kept_session_emu(emu_lib, name):
    ah.check_session(DEV, name)
