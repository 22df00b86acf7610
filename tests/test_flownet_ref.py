"""The FlowNet2 teacher's three native operators pinned to the reference's OWN kernel code: oracle/build_ref.py compiles the
`__global__` templates of correlation_cuda_kernel.cu / resample2d_kernel.cu / channelnorm_kernel.cu for the host from the
reference tree (SIMT fibre emulator underneath, launch geometry of the reference's host wrappers) into
oracle/_ref/libflownet2_ref.so.  Held to it here: the Python restatement (oracle/flownet_oracle.py), the HIP kernels of
csrc/flownet_ops.hip on the emulator, and the HIP kernels on the MI355X.  Where that library can be neither loaded nor built, the
checker is tests/golden/flownet2_ref_kernels.npz: the library's outputs on the seeded inputs of these tests, recorded by
`python tests/test_flownet_ref.py` (which needs the library); where the library is present, every call is also held to the
recording."""
import hashlib
import os

import numpy as np
import pytest
import torch

import op_checks as oc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'flownet2_ref_kernels.npz')
OPS = ('correlation', 'resample2d', 'channelnorm')


def _key(op, args):
    h = hashlib.sha1(op.encode())
    for a in args:
        h.update(a.detach().contiguous().float().numpy().tobytes() if torch.is_tensor(a) else repr(a).encode())
    return '%s_%s' % (op, h.hexdigest()[:24])


class _Checker:
    """the reference kernels through `live` (oracle.flownet_ref) or, with live=None, from the recording; record=True collects
    the live outputs for a new recording instead of comparing them with the stored one"""

    def __init__(self, live, record=False):
        self.live, self.record, self.out = live, record, {}
        self.stored = np.load(GOLDEN) if (os.path.exists(GOLDEN) and not record) else None
        assert live is not None or self.stored is not None, 'no reference kernels and no recording of them (%s)' % GOLDEN

    def _call(self, op, *args):
        key = _key(op, args)
        if self.live is None:
            assert key in self.stored.files, 'inputs of this %s call were not recorded: re-run tests/test_flownet_ref.py' % op
            return torch.from_numpy(self.stored[key].copy())
        got = getattr(self.live, op)(*args)
        if self.record:
            self.out[key] = got.numpy().copy()
        elif self.stored is not None:
            assert key in self.stored.files and np.array_equal(self.stored[key], got.numpy()), 'recording out of date: %s' % op
        return got

    def correlation(self, *args):
        return self._call('correlation', *args)

    def resample2d(self, *args):
        return self._call('resample2d', *args)

    def channelnorm(self, *args):
        return self._call('channelnorm', *args)


def _ref(record=False):
    from oracle import flownet_ref
    return _Checker(flownet_ref if flownet_ref.load() is not None else None, record)


def test_restatement_equals_the_reference_kernels():
    _check_restatement(_ref())


def _check_restatement(R):
    from oracle import flownet_oracle as FO
    g = torch.Generator().manual_seed(404)
    # FlowNetC's configuration (FlowNetC.py:28-31: pad 20, kernel 1, displacement 20, strides 1 / 2) and odd geometries
    for (n, c, h, w, pad, md, s1, s2) in [(1, 256, 6, 10, 20, 20, 1, 2), (2, 70, 9, 37, 20, 20, 1, 2), (1, 64, 12, 40, 4, 4, 1, 1),
                                           (1, 5, 11, 13, 6, 6, 2, 3)]:
        f1, f2 = torch.randn(n, c, h, w, generator=g), torch.randn(n, c, h, w, generator=g)
        a, b = R.correlation(f1, f2, pad, 1, md, s1, s2), FO.correlation(f1, f2, pad, 1, md, s1, s2)
        assert a.shape == b.shape
        assert float((a - b).abs().max()) <= 1e-6 * max(float(a.abs().max()), 1.0)        # summation order over the channels
    for (n, c, h, w, mag) in [(2, 3, 17, 23, 6.0), (1, 2, 8, 64, 80.0), (1, 3, 33, 31, 2.5)]:
        img = torch.randn(n, c, h, w, generator=g)
        flow = (torch.rand(n, 2, h, w, generator=g) - 0.5) * mag
        flow[:, :, 0] = torch.round(flow[:, :, 0])
        assert torch.equal(R.resample2d(img, flow), FO.resample2d(img, flow))              # bit for bit
    for shp in [(2, 7, 5, 9), (1, 3, 16, 16), (1, 2, 4, 4)]:
        x = torch.randn(*shp, generator=g) * 3
        assert torch.equal(R.channelnorm(x), FO.channelnorm(x))


def test_emulated_hip_kernels_equal_the_reference_kernels(emu_lib):
    oc.check_flownet_ops(torch.device('cpu'), checker=_ref())


@pytest.mark.gpu
def test_hip_kernels_equal_the_reference_kernels(hip_lib):
    oc.check_flownet_ops(torch.device('cuda:0'), seed=19, checker=_ref())


if __name__ == '__main__':
    # (re)record the checker: the three tests' calls on the host - the emulated HIP library stands in for the device kernels
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ['FSV2V_EMU'] = '1'
    from importlib import import_module
    import fsv2v_amd  # noqa: F401
    import_module('few-shot-vid2vid_amd.build').build_emu()
    rec = _ref(record=True)
    assert rec.live is not None, 'recording needs oracle/_ref/libflownet2_ref.so (oracle/build_ref.py)'
    _check_restatement(rec)
    oc.check_flownet_ops(torch.device('cpu'), checker=rec)
    oc.check_flownet_ops(torch.device('cpu'), seed=19, checker=rec)
    np.savez_compressed(GOLDEN, **rec.out)
    print(GOLDEN, len(rec.out), 'calls', os.path.getsize(GOLDEN), 'bytes')
