"""Shared checks of the adaptation-target kernel of the test-time finetune (csrc/roll_flip.hip through ops.roll_flip): bit for bit
against the `torch.cat` / `torch.flip` form of the loop in `Vid2VidModel.finetune`, the draw parameters read from device memory, the
clamped / modulo definition for out-of-range integers, and the refusals.  Used by tests/test_finetune_graph_emu.py (emulator) and
tests/test_finetune_graph_gpu.py (hardware).

Importing this module lists the new entry point in the ledger of tests/test_entry_point_coverage.py, the way tests/attn_half_checks.py
does: that file is a yardstick and is not edited, and collection imports every test module before anything runs."""
import torch

import infer_session_checks as ic
import test_entry_point_coverage as ledger

ledger.CHECKED_BY.update({
    'fsv_roll_flip': 'finetune_graph_checks.check_roll_flip',
})

_mod = ic._mod
B, N, CS = 2, 3, (3, 5)                 # label-like and image-like channel counts in ONE launch
SIZES = [(16, 24), (9, 7)]


# ------------------------------------------------------------------------------------------------ (a) the kernel
def roll_ref(t, ny, nx, flip):
    """`roll` of Vid2VidModel.finetune (util/util.py:157-168), on a [B, C, H, W] tensor"""
    t = torch.cat([t[:, :, -ny:], t[:, :, :-ny]], dim=2)
    t = torch.cat([t[:, :, :, -nx:], t[:, :, :, :-nx]], dim=3)
    return torch.flip(t, dims=[3]) if flip else t


def _stacks(h, w, seed=5):
    g = torch.Generator().manual_seed(seed + h * w)
    return [torch.randn(B, N, c, h, w, generator=g) for c in CS]


def _params(device, row):
    return torch.tensor([int(v) for v in row], dtype=torch.int32).to(device)


def draw_rows(h, w):
    return [(idx, ny, nx, flip) for idx in (0, N - 1) for ny in (0, 1, h - 1, h) for nx in (0, 1, w - 1, w) for flip in (0, 1)]


def check_roll_flip(device, h, w):
    """every row of the grid: both tensors of one launch equal the cat / flip form, bit for bit; dense NCHW outputs"""
    ops = _mod('ops')
    stacks = _stacks(h, w)
    dev = [t.to(device) for t in stacks]
    for row in draw_rows(h, w):
        idx, ny, nx, flip = row
        outs = ops.roll_flip(dev, _params(device, row))
        assert len(outs) == 2
        for t, o in zip(stacks, outs):
            assert tuple(o.shape) == (B, t.shape[2], h, w) and o.is_contiguous() and o.dtype == torch.float32
            want = roll_ref(t[:, idx], ny, nx, bool(flip))
            assert torch.equal(o.cpu(), want), (row, t.shape[2])
    one = ops.roll_flip(dev[:1], _params(device, (1, 1, 1, 1)))              # a single stack: the second tensor is not read
    assert len(one) == 1 and torch.equal(one[0].cpu(), roll_ref(stacks[0][:, 1], 1, 1, True))


def check_params_are_read_on_the_device(device):
    """two calls with IDENTICAL arguments, the parameter buffer overwritten in between: the second call gives the second target"""
    ops = _mod('ops')
    h, w = SIZES[0]
    stacks = _stacks(h, w)
    dev = [t.to(device) for t in stacks]
    params = _params(device, (0, 1, w - 1, 0))
    first = [o.clone() for o in ops.roll_flip(dev, params)]
    params.copy_(_params(device, (2, h - 1, 1, 1)))
    second = ops.roll_flip(dev, params)
    for t, a, b in zip(stacks, first, second):
        assert torch.equal(a.cpu(), roll_ref(t[:, 0], 1, w - 1, False))
        assert torch.equal(b.cpu(), roll_ref(t[:, 2], h - 1, 1, True))
        assert not torch.equal(a, b)


def check_out_of_range_params(device):
    """idx is clamped into [0, N), ny / nx are taken modulo H / W (negative values included), flip is != 0: the definition of the
    header.  Every index stays inside the tensors."""
    ops = _mod('ops')
    for h, w in SIZES:
        stacks = _stacks(h, w)
        dev = [t.to(device) for t in stacks]
        for row, (idx, ny, nx, flip) in (((N + 5, -3, 3 * w + 1, 7), (N - 1, h - 3, 1, True)),
                                         ((-4, 2 * h, -w - 2, -1), (0, 0, w - 2, True)),
                                         ((1, -h, 0, 0), (1, 0, 0, False))):
            outs = ops.roll_flip(dev, _params(device, row))
            for t, o in zip(stacks, outs):
                assert torch.equal(o.cpu(), roll_ref(t[:, idx], ny, nx, flip)), row


def check_refusals(device):
    import pytest
    ops, lib = _mod('ops'), _mod('lib')
    h, w = SIZES[1]
    dev = [t.to(device) for t in _stacks(h, w)]
    params = _params(device, (0, 0, 0, 0))
    with pytest.raises(ValueError, match='forward-only'):
        ops.roll_flip([dev[0].clone().requires_grad_(True), dev[1]], params)
    with pytest.raises(ValueError):
        ops.roll_flip(dev, params.long())
    with pytest.raises(ValueError):
        ops.roll_flip([dev[0], dev[1][:, :2]], params)
    bad = lib.ENUMS['FSV_ERR_BAD_ARG']
    out = torch.zeros(B, CS[0], h, w, device=device)
    call = lambda *a: lib.call_status('fsv_roll_flip', *a, lib.stream_ptr())
    assert call(lib.ptr(dev[0]), lib.ptr(out), CS[0], None, None, 0, B, N, h, w, None) == bad
    assert call(lib.ptr(dev[0]), lib.ptr(out), CS[0], None, None, 2, B, N, h, w, lib.ptr(params)) == bad
    assert call(lib.ptr(dev[0]), lib.ptr(out), CS[0], None, None, 0, B, 0, h, w, lib.ptr(params)) == bad
    assert float(out.abs().max()) == 0.0
