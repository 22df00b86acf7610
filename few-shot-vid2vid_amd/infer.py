"""Frozen-weight video inference: prepare once, replay one graph per frame.

`Vid2VidModel.inference` (test.py:39-41) runs every frame as if the weights could change between frames.  At test time they cannot,
and about half of an eager frame's launches recompute constants: the K-major layouts of every shared weight (there is no
optimiser, hence no layout_cache.LayoutCache), sigma of every spectral layer, the [gamma | beta] operands of every SPADE site, the
reference encoder's down path, the (mean, rstd) pair of every eval-mode BatchNorm.  An `InferenceSession` takes them once and keeps
them until it is told that the weights changed:

    sess = InferenceSession(model, opt, fold_norms=False, frames_u8=False, warmup=1, keep_references=False, inputs_u8=False,
                            fused_attention=False)
    out = sess(tgt_label, ref_labels, ref_images)     # one frame: the six tensors of model.inference() (+ out.image_u8)
    sess.reset()                                      # between sequences (new references allowed)
    sess.refreeze()                                   # after anything changed the parameters or buffers
    sess.close()                                      # detach everything the session hung on the model

What is frozen and where it lives (everything belongs to the session: `close()` leaves the model as it found it)

  * layouts     `FrozenWeights.layout`, reached from ops._ConvFn through `weight._fsv_frozen`: the re-arrangement the un-cached eager
                path issues on every call (1 / sigma baked in, ops.py `prep_weight(w4, 0, geom, scale=inv)`), built by the FIRST
                eager call that meets the weight - the geometry (stride, channel padding, operand precision) is only known there -
                and never inside a capture.  Parameters an optimiser's LayoutCache owns (`--finetune`) keep that cache.
  * sigma       `module._sig_frozen`: one `SpectralState.update(..., training=False)` per spectral layer.
  * SPADE       `FrozenWeights.spade_*`, reached from ops._SpadeFn: the operands of fixed weights and of the generated weights kept
                for the sequence, keyed by the weight tensors themselves (no global table, no epoch: a pass outside the session can
                never find them stale).  The 3x3 form (--spade_ks 3) prepares per call as before.
  * BatchNorm   `running_mean._fsv_frozen_stats`: (mean, rstd) of eval-mode layers, validated by the buffers' versions.

Once per sequence (n_shot == 1): frame 0 runs `model.inference()` eagerly - with `--finetune` on the live weights, the session
refreezes behind it - and leaves in static buffers the generated embed_w / norm_w / conv_w and the deepest reference feature x;
`reset()` + a new frame 0 rewrites the same buffers in place (and the operands prepared from them), so a captured graph stays valid
across sequences.  With n_shot > 1 reference encoding and attention depend on the frame and stay in the per-frame work - unless

keep_references=True (n_shot > 1; a no-op with one reference): the reference side of the sequence is READ AT FRAME 0 AND KEPT.  In
eval() every layer of the reference encoders is per sample (BatchNorm takes its running buffers, InstanceNorm is per sample
anyway), so a reference's features up to the attention level and its keys depend on neither the frame nor the other inputs.  While
frame 0 runs - model.inference() itself, eager and unchanged - the session collects the two kinds of operand the attention reads
from the reference side, the key encoding of the reference labels (`kmat`) and the outputs of ref_img_down_{A-1} / ref_label_down_{A-1}
(`xmat`; A = n_downsample_A), in the arrangement the GEMMs read, into static buffers of its own (`KeptReferences`); their K-major
layouts are frozen like those of any other constant weight.  A steady frame then runs the query encoder, the energy GEMM, the
softmax, the weighted sums and everything behind them (encoder levels A .. n-1, up path, pooled products, MLP bank, weight
generation: they depend on the current label) on the same values, hence with the same bits; the mass per reference (atn_vis,
ref_idx) comes out of the softmax launch (ops.softmax_channels groups) instead of two more reductions of the attention tensor, so
atn_vis differs from the eager path's by the order of one fp32 sum.  THE DIFFERENCE TO model.inference(): that one re-reads
ref_labels / ref_images on every frame; a session that keeps them ignores what is passed for them on frames t >= 1 (which is why
the flag is opt-in).  reset() + a new frame 0 of equal shapes refills the buffers in place: the graph survives.  refreeze() drops
them with the graph, and the next call is a frame 0.

fused_attention=True (n_shot > 1): every frame of the session - frame 0, the eager warm-up and the captured steady frame - runs the
attention as the one streaming launch of ops.attention_fused (csrc/attention.hip; a graph node like any other): no energy /
attention tensor, no band loop, no band buffer.  With keep_references the session then keeps the key encoding and the reference
features as the encoders wrote them (their own NHWC memory: `KeptReferences.key` / `.vals`), which is what that kernel reads, and
no kmat / xmat arrangement with its K-major layouts.  Not bit-equal to the eager frames: the summation order of the softmax and of
the weighted sums changes (a shape the kernel does not serve runs the launches above).  The mark sits on netG until close()
(like the kept reference side): model.inference() or another session on the same model is fused too while this one is attached.

fused_attention='half' (n_shot > 1): as above with the attention on the f16 matrix cores (ops.attention_fused_half,
csrc/attention_h.hip: energies from split half operands - about 22 bits -, plain half probabilities and values, fp32 softmax and
accumulation) wherever that kernel serves the shape - every channel count a multiple of 8 up to 128 -, the fp32 streaming launch
elsewhere.  With keep_references the session keeps the PREPARED operands (`KeptReferences.half`: the two half planes of the keys,
the half key-contiguous value maps - half the memory of the fp32 maps, the same for the keys) and a steady frame issues the query
encoder, one fsv_attention_fused_fwd_h and the finishing launch: no prep, no cast, no arrangement.  Without keep_references the
prep launch runs per frame, in the captured graph.

inputs_u8=True: the three inputs arrive as uint8 with the channel last ([B, 1, H, W, C] / [B, N, H, W, C]), as a video pipeline
delivers them, and are converted on the device into the session's static inputs (ops.image_from_u8: the dataset's ToTensor +
Normalize(0.5, 0.5), bit-exact).  Class-index label maps (label_nc != 0) are not covered: the flag raises for them.

Replay (frames t >= 1): the conventions of graph_step.GraphedIteration - static input buffers, outputs as static tensors, the first
`warmup` steady frames eager (they build what is built lazily), then ONE captured graph; a failed capture is recorded in
`capture_failures` and the session goes on eagerly; on the emulator the same body runs eagerly on the static buffers.  The
previous-frame buffers are a device ring of depth n_frames_G - 1 that the graph itself advances.

fold_norms=True: convolution -> eval-mode affine BatchNorm -> LeakyReLU as ONE launch where nothing else reads the convolution's
output (SPADEConv2d, FlowGenerator's normed layers, conv_0 -> bn_1 of a block without SPADE): s = gamma rsqrt(var + eps) / sigma and
t = (bias - mean) gamma rsqrt(var + eps) + beta in float64, stored as fp32; the layout carries s in its columns (`fsv_prep_weight`
col_scale) and the launch is the gather-GEMM with bias = t, act = LeakyReLU.  Not bit-equal to the two launches (one multiply per
weight and one add per output are re-associated); `folded_sites` lists the layers.

frames_u8=True: the generated frame also as [B, H, W, 3] uint8 (`out.image_u8`, ops.image_u8: tensor2im's arithmetic, bit-exact).
"""
import torch
import torch.nn as nn

from . import conv, lib, networks, ops
from .conv import prep_weight


def _capturing():
    return (not lib.is_emu()) and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class _Layout:
    __slots__ = ("weight", "state", "fwd", "up_fwd", "baked", "w4s", "rebuild", "owner")

    def can_grow(self):
        return not _capturing()


class _SpadeOps:
    __slots__ = ("tensors", "key", "ops", "issue")


class FrozenWeights:
    """the session's own caches of operands derived from weights that do not change (see the module docstring)"""

    def __init__(self):
        self.layouts = {}
        self.spade = {}
        self.fold_scale = {}          # id(weight) -> (weight, per-output-channel factors) of a folded BatchNorm

    # ---------------------------------------------------------------------------------------------- convolution layouts
    def layout(self, weight, w4, geom, cpad, half, inv):
        """the forward operand of ops._ConvFn's un-cached path for this call, or None (the call then re-arranges itself)"""
        fold = self.fold_scale.get(id(weight))
        if fold is not None and fold[0] is not weight:
            fold = None
        if fold is not None and inv is not None:
            return None                   # a folded weight called with its own sigma: not the folded site
        key = (id(weight), tuple(w4.shape), geom.kh, geom.kw, geom.stride, geom.pad, cpad, bool(half),
               inv.data_ptr() if inv is not None else 0)
        e = self.layouts.get(key)
        state = (weight._version, weight.data_ptr())
        if e is not None and e.weight is weight and e.state == state:
            return e
        if _capturing():
            return None                   # nothing is built inside a capture
        e = _Layout()
        e.weight, e.state, e.up_fwd, e.w4s, e.owner = weight, state, None, None, self
        w4p = torch.nn.functional.pad(w4, (0, 0, 0, 0, 0, cpad)) if cpad else w4
        if fold is not None:
            wt, _, ldw = prep_weight(w4p, 0, geom, col_scale=fold[1])
            e.baked = True
            e.w4s = w4 * fold[1].view(-1, 1, 1, 1)
            e.rebuild = None
        else:
            # (half path: W itself is rounded and 1 / sigma applied to the fp32 accumulator - ops._ConvFn's own rule)
            scale = None if half else inv
            wt, _, ldw = prep_weight(w4p, 0, geom, scale=scale)
            e.baked = not half
            e.rebuild = (lambda: prep_weight(w4p, 0, geom, scale=scale, out=wt)) if not cpad else None
        e.fwd = (wt, ldw)
        self.layouts[key] = e
        return e

    # ---------------------------------------------------------------------------------------------- SPADE operands
    def spade_get(self, wg, key):
        e = self.spade.get(id(wg))
        if e is None or e.tensors[0] is not wg:
            return None
        return (e.key, e.ops)

    def spade_put(self, tensors, key, operands, issue):
        if _capturing():
            return
        e = _SpadeOps()
        e.tensors, e.key, e.ops, e.issue = tuple(tensors), key, operands, issue
        self.spade[id(tensors[0])] = e

    # ---------------------------------------------------------------------------------------------- refill
    def refill(self):
        """the per-sample (generated) weights were rewritten in place: rewrite what was prepared from them, in place as well"""
        for key, e in list(self.layouts.items()):
            if e.weight.dim() == 5:
                if e.rebuild is None or e.state[1] != e.weight.data_ptr():
                    del self.layouts[key]
                    continue
                e.rebuild()
                e.state = (e.weight._version, e.weight.data_ptr())
        for e in self.spade.values():
            if e.tensors[0].dim() == 5:
                e.issue()
                e.key = (e.key[0],) + tuple(t._version for t in e.tensors) + tuple(e.key[5:])


def fold_conv_bn(frozen, cv, bn, eps=1e-5):
    """fold the eval-mode affine BatchNorm `bn` (and LeakyReLU) into the networks.Conv2d `cv` whose output it alone reads:
        s[co] = gamma rsqrt(running_var + eps) / sigma        -> the columns of the frozen layout (fsv_prep_weight col_scale)
        t[co] = (bias - running_mean) gamma rsqrt(running_var + eps) + beta        -> the launch's bias
    in float64, stored as fp32.  cv's weight must be tagged with `frozen` and, if spectral, carry its frozen sigma."""
    w = cv.weight_orig if cv.spectral else cv.weight
    with torch.no_grad():
        r = bn.weight.detach().double() * torch.rsqrt(bn.running_var.detach().double() + eps)
        s = r / cv._sig_frozen[0].double() if cv.spectral else r
        b = cv.bias.detach().double() if cv.bias is not None else 0.0
        t = (b - bn.running_mean.detach().double()) * r + bn.bias.detach().double()
        frozen.fold_scale[id(w)] = (w, s.float().contiguous())
        cv._fsv_fold = (t.float().contiguous(), bn)


def count_graph_nodes(graph):
    """{node kind: count} of a torch.cuda.CUDAGraph captured with keep_graph=True (hipGraphGetNodes / hipGraphNodeGetType)"""
    import collections
    import ctypes
    hip = ctypes.CDLL('libamdhip64.so')
    raw = ctypes.c_void_p(graph.raw_cuda_graph())
    n = ctypes.c_size_t(0)
    if hip.hipGraphGetNodes(raw, None, ctypes.byref(n)) != 0:
        return None
    arr = (ctypes.c_void_p * max(n.value, 1))()
    if hip.hipGraphGetNodes(raw, arr, ctypes.byref(n)) != 0:
        return None
    names = {0: 'kernel', 1: 'memcpy', 2: 'memset', 3: 'host', 4: 'graph', 5: 'empty', 6: 'wait_event', 7: 'event_record'}
    kinds = collections.Counter()
    for node in arr[:n.value]:
        t = ctypes.c_int(-1)
        hip.hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(t))
        kinds[names.get(t.value, 'type%d' % t.value)] += 1
    return dict(kinds)


class KeptReferences:
    """the reference side of one sequence, owned by an InferenceSession (keep_references): netG._kept_refs.  After a fused frame 0
    (fused_attention) it is `key` [b n, c, h, w] and `vals` = [image encoder's, label encoder's (not under 'concat')] [b n, cv, h, w],
    dense NHWC clones of the encoders' outputs - what ops.attention_fused reads - and kmat / xmats / band stay empty; no layout is
    frozen for them.  Otherwise: `collect` takes what
    frame 0's attention_module hands it; `keep` copies that into the static buffers kmat [b, n*hw, c, 1, 1] and xmats = [image
    encoder's, label encoder's (not under 'concat')] [b, c, n*hw, 1, 1] - the per-sample 1x1 "weights" of the two attention GEMMs -
    allocating them or, for equal shapes, rewriting them in place (-> True: the old buffers, and a graph captured over them,
    stay valid)."""

    def __init__(self):
        self.ready, self.kmat, self.xmats = False, None, []
        self.key, self.vals = None, []           # a fused frame 0 (ops.attention_fused): the encoders' outputs as they lie in memory
        self.half = None                         # a half frame 0 (ops.attention_fused_half): ops.AttentionHalfOperands, the session's own
        self._got = None
        self.band = None

    def band_buffer(self, numel, device):
        """the one energy / attention band of a banded attention (networks.AttentionBands.attend): the session's, like the other
        static buffers - allocated by the eager warm-up frame, the same memory on every replay (the plan, and with it the size, is
        fixed by the shapes the graph was captured for; other shapes drop the graph and this buffer together)"""
        if self.band is None or self.band.numel() < numel or self.band.device != device:
            self.band = torch.empty(numel, dtype=torch.float32, device=device)
        return self.band

    def begin(self):
        self.ready, self._got = False, {}

    def collect(self, name, t):
        if self._got is not None:
            self._got[name] = t                     # (the last pass wins: --finetune runs adaptation passes before the frame's own)

    def abort(self):
        self._got = None

    def keep(self, frozen):
        got, self._got = self._got, None
        if got and 'half' in got and 'half_val0' in got:
            return self._keep_half(got)
        fused = bool(got) and 'key' in got and 'val0' in got
        if not fused and (not got or 'kmat' not in got or 'xmat0' not in got):
            raise RuntimeError("keep_references: frame 0 did not pass through the attention module")
        if fused:
            new = [got['key']] + [got[k] for k in ('val0', 'val1') if k in got]
            old = ([self.key] + self.vals) if self.key is not None else []
        else:
            new = [got['kmat']] + [got[k] for k in ('xmat0', 'xmat1') if k in got]
            old = ([self.kmat] + self.xmats) if self.kmat is not None else []
        same = len(old) == len(new) and all(a.shape == b.shape and a.device == b.device for a, b in zip(old, new))
        if same:
            for dst, src in zip(old, new):
                dst.copy_(src)
        elif fused:
            old = [ops.to_nhwc(t.detach()).clone() for t in new]           # (clone keeps the dense NHWC strides)
            self.key, self.vals, self.kmat, self.xmats, self.band, self.half = old[0], old[1:], None, [], None, None
        else:
            old = [t.detach().clone(memory_format=torch.contiguous_format) for t in new]
            self.kmat, self.xmats, self.key, self.vals, self.half = old[0], old[1:], None, [], None
        if not fused:                            # (the fused kernel reads the kept tensors themselves: no layout to freeze)
            for t in old:
                t._fsv_frozen = frozen
        self.ready = True
        return same

    def _keep_half(self, got):
        """a half frame 0: the prepared operands (half planes of the keys, half key-contiguous value maps - a second map that was
        not announced came from a later call) into the session's own, rewritten in place for equal shapes; nothing else is kept"""
        src = got['half']
        vts = [got['half_val0']] + ([got['half_val1']] if 'half_val1' in got else [])
        new = [src.kh, src.kl] + vts
        old = self.half.tensors() if self.half is not None else []
        same = len(old) == len(new) and all(a.shape == b.shape and a.device == b.device for a, b in zip(old, new))
        if same:
            for dst, s in zip(old, new):
                dst.copy_(s)
        else:
            own = [t.detach().clone() for t in new]
            self.half = ops.AttentionHalfOperands(own[0], own[1], own[2:], src.b, src.n, src.p, src.c, [t.shape[1] for t in vts],
                                                  src.nps)
            self.key, self.vals, self.kmat, self.xmats, self.band = None, [], None, [], None
        self.ready = True
        return same

    def drop(self):
        self.ready, self.kmat, self.xmats, self._got, self.band = False, None, [], None, None
        self.key, self.vals, self.half = None, [], None


class FrameOutputs(tuple):
    """(fake, raw, warped, flow, mask, atn_score) of Vid2VidModel.inference; `image_u8` ([B, H, W, 3] uint8) with frames_u8"""
    image_u8 = None


def _map_tensors(obj, fn):
    if torch.is_tensor(obj):
        return fn(obj)
    if isinstance(obj, (list, tuple)):
        return type(obj)(_map_tensors(o, fn) for o in obj)
    return obj


def _flat_tensors(obj, out=None):
    out = [] if out is None else out
    if torch.is_tensor(obj):
        out.append(obj)
    elif isinstance(obj, (list, tuple)):
        for o in obj:
            _flat_tensors(o, out)
    return out


class InferenceSession:
    def __init__(self, model, opt, fold_norms=False, frames_u8=False, warmup=1, keep_references=False, inputs_u8=False,
                 fused_attention=False):
        model = getattr(model, 'module', model)
        if model.training:
            raise RuntimeError("InferenceSession freezes the weights: put the model in eval() first (it is in train() mode)")
        if getattr(opt, 'isTrain', False):
            raise RuntimeError("InferenceSession is the test.py path: opt.isTrain must be False (the generated weights of frame 0 "
                               "are kept for the sequence)")
        self.model, self.opt = model, opt
        self.fold_norms, self.frames_u8 = bool(fold_norms), bool(frames_u8)
        self.inputs_u8 = bool(inputs_u8)
        if self.inputs_u8 and getattr(opt, 'label_nc', 0) != 0:
            raise ValueError("inputs_u8 converts image-like labels (pose, face sketches); class-index label maps (label_nc = %d) "
                             "are not covered" % opt.label_nc)
        netG = model.netG
        # keep_references: only where there is an attention module to feed (n_shot > 1); with one reference the flag is a no-op
        self.keep_references = bool(keep_references) and netG.n_shot > 1 and 1 <= netG.n_downsample_A <= netG.n_downsample_G
        self._kept = KeptReferences() if self.keep_references else None
        self.warmup = max(int(warmup), 1)      # at least one eager steady frame: it builds what the capture may not
        self.capture_failures = []             # (signature, first line of the error) of every capture that fell back to eager frames
        self.n_captures = 0
        self.folded_sites = []
        self._emulated = lib.emu_requested()
        if not self._emulated and not torch.cuda.is_available():
            raise RuntimeError("InferenceSession needs a GPU (hipGraph capture)")
        self.frozen = None
        self._tagged = []
        if self._kept is not None:
            netG._kept_refs = self._kept
        # fused_attention: the mark networks.attention_fused_switch reads, on netG for as long as the session is attached
        # 'half': also the mark networks.attention_half_switch reads - the half kernel where it serves the shape, the fp32 one elsewhere
        if fused_attention not in (False, True, 'half'):
            raise ValueError("fused_attention=%r: False, True or 'half' expected" % (fused_attention,))
        self.fused_attention = bool(fused_attention) and netG.n_shot > 1
        self.half_attention = self.fused_attention and fused_attention == 'half'
        if self.fused_attention:
            netG._attn_fused = True
        if self.half_attention:
            netG._attn_half = True
        self._drop_graph()
        self._drop_buffers()
        self._sig = None
        self.t = None
        self._attach()

    # ------------------------------------------------------------------------------------------------ freeze
    def _nets(self):
        return [n for n in (self.model.netG, getattr(self.model, 'netGf', None)) if n is not None]

    def _attach(self):
        fz = self.frozen = FrozenWeights()
        self._spectral, self._bn_buffers, self._folded = [], [], []
        with torch.no_grad():
            for net in self._nets():
                for p in net.parameters():
                    if getattr(p, '_fsv_cache', None) is None:      # (an optimiser's LayoutCache keeps what it owns: --finetune)
                        p._fsv_frozen = fz
                        self._tagged.append(p)
                for m in networks.spectral_layers(net):
                    m._sig_frozen = ops.SpectralState.update(m.weight_orig, m.weight_u, m.weight_v, False)
                    self._spectral.append(m)
                for m in net.modules():
                    if isinstance(m, networks.BatchNorm):
                        rm, rv = m.running_mean, m.running_var
                        pair = (rm.detach().clone(), torch.rsqrt(rv.detach() + 1e-5))
                        rm._fsv_frozen_stats = ((rm._version, rv._version, rv.data_ptr(), 1e-5), pair)
                        self._bn_buffers.append(rm)
            self.folded_sites = self._fold() if self.fold_norms else []
        for t in _flat_tensors(self._static_w):
            t._fsv_frozen = fz
        if self._kept is not None and self._kept.kmat is not None:
            for t in [self._kept.kmat] + self._kept.xmats:
                t._fsv_frozen = fz

    def _fold_candidates(self, net):
        for name, m in net.named_modules():
            if isinstance(m, networks.SPADEConv2d):
                yield name + '.conv', m.conv, m.bn
            elif isinstance(m, networks.FlowGenerator):
                for seq_name in ('down_flow', 'up_flow'):
                    for k, layer in enumerate(getattr(m, seq_name)):
                        if isinstance(layer, nn.ModuleList) and len(layer) == 2 and isinstance(layer[0], networks.Conv2d):
                            yield '%s.%s.%d.0' % (name, seq_name, k), layer[0], layer[1]
            elif isinstance(m, networks.SPADEResnetBlock) and not m.spade and not m.conv_params_free:
                yield name + '.conv_0', m.conv_0, m.bn_1

    def _fold(self):
        """conv -> eval-mode affine BatchNorm -> LeakyReLU where the BatchNorm is the only reader: s into the layout's columns, t as
        the bias (float64 arithmetic, fp32 storage)"""
        sites, seen = [], set()
        for net in self._nets():
            for name, cv, bn in self._fold_candidates(net):
                w = cv.weight_orig if cv.spectral else cv.weight
                if (id(cv) in seen or not isinstance(bn, networks.BatchNorm) or not bn.affine or
                        getattr(w, '_fsv_cache', None) is not None):
                    continue
                seen.add(id(cv))
                fold_conv_bn(self.frozen, cv, bn)
                self._folded.append(cv)
                sites.append(name)
        return sites

    def _detach(self):
        for p in self._tagged:
            if getattr(p, '_fsv_frozen', None) is not None:
                del p._fsv_frozen
        self._tagged = []
        for t in _flat_tensors(self._static_w):
            if getattr(t, '_fsv_frozen', None) is not None:
                del t._fsv_frozen
        if self._kept is not None and self._kept.kmat is not None:
            for t in [self._kept.kmat] + self._kept.xmats:
                if getattr(t, '_fsv_frozen', None) is not None:
                    del t._fsv_frozen
        for m in self._spectral:
            m._sig_frozen = None
        for rm in self._bn_buffers:
            if getattr(rm, '_fsv_frozen_stats', None) is not None:
                del rm._fsv_frozen_stats
        for cv in self._folded:
            cv._fsv_fold = None
        self._spectral, self._bn_buffers, self._folded = [], [], []
        self.frozen = None

    def refreeze(self):
        """after anything changed the parameters or buffers (load_state_dict, a finetune): take every constant again.  The captured
        graph read the old ones and is dropped; within a running sequence the reference feature is recomputed per frame, as the
        eager path does, until the next frame 0 keeps it again.  With keep_references the kept reference side was encoded by the
        old weights: it is dropped, and the next call is a frame 0."""
        self._detach()
        self._drop_graph()
        self.model.netG._frozen_x = None
        if self._kept is not None:
            self._kept.drop()
            self.reset()
        self._attach()

    def close(self):
        """detach everything the session hung on the model; the model's own inference state starts a new sequence"""
        self._detach()
        self._drop_graph()
        self.model.netG._frozen_x = None
        if self._kept is not None:
            self._kept.drop()
            if self.model.netG.__dict__.get('_kept_refs') is self._kept:
                del self.model.netG._kept_refs
        if self.fused_attention:
            self.model.netG.__dict__.pop('_attn_fused', None)
            self.model.netG.__dict__.pop('_attn_half', None)
        self._drop_buffers()
        if getattr(self.model, '_infer_session', None) is self:
            self.model._infer_session = None
        self.model.reset_inference()
        self.t = None

    def reset(self):
        """between sequences: the next call is a frame 0 (new reference images allowed)"""
        self.t = None
        self.model.reset_inference()

    # ------------------------------------------------------------------------------------------------ bookkeeping
    def _drop_graph(self):
        """forget the captured frame (the static input / ring buffers stay: a running sequence goes on from them)"""
        self._graph, self._graph_has_x, self._out, self._steady, self._eager_only = None, False, None, 0, False

    def _drop_buffers(self):
        self._in = self._ring = self._static_w = self._static_x = self._ref_in = None
        if getattr(self, '_kept', None) is not None:
            self._kept.drop()

    keep_graph = False       # tools/infer_session.py sets it before the capture: the hipGraph stays queryable (graph_nodes)

    def graph_nodes(self):
        """{node kind: count} of the captured frame (needs `keep_graph`), or None"""
        return count_graph_nodes(self._graph) if (self._graph is not None and self.keep_graph) else None

    def launch_mode(self):
        if self.capture_failures:
            return 'eager fallback (hipGraph capture failed: %s)' % self.capture_failures[-1][1]
        if self._emulated:
            return 'emulated kernels, eager'
        return 'hipgraph' if self._graph is not None else 'eager (warm-up)'

    @staticmethod
    def _signature(tensors):
        return tuple((tuple(t.shape), t.dtype, str(t.device)) for t in tensors)

    # ------------------------------------------------------------------------------------------------ frame 0
    def _frame0(self, tgt_label, ref_labels, ref_images):
        model, netG = self.model, self.model.netG
        model.reset_inference()
        netG._frozen_x = None
        sig = self._signature((tgt_label, ref_labels, ref_images))
        if sig != self._sig:                     # other shapes: nothing captured or kept for the old ones applies
            self._drop_graph()
            self._drop_buffers()
            self._sig = sig
        finetune = bool(getattr(self.opt, 'finetune', False))
        if finetune:
            self._detach()                       # the adaptation steps train on the live weights
            self._drop_graph()
        kept = self._kept
        if self.inputs_u8:
            tgt_label = ops.image_from_u8(tgt_label)
        if kept is not None or self.inputs_u8:
            # the references of the sequence in static buffers of the session's own: the steady frames read them there
            ref_labels, ref_images = self._hold_references(ref_labels, ref_images)
        if kept is not None:
            kept.begin()                         # (not ready: frame 0 is the eager path, which hands its operands to `kept`)
        try:
            out = model.inference(tgt_label, ref_labels, ref_images)
        except BaseException:
            if kept is not None:
                kept.abort()
            raise
        finally:
            if finetune:
                self._attach()
        with torch.no_grad():
            if netG.n_shot == 1 and ref_labels.shape[1] == 1:
                self._keep_sequence()
            if kept is not None:
                if kept.keep(self.frozen):
                    self.frozen.refill()         # rewritten in place: so are the layouts prepared from them
                elif self._graph is not None:
                    self._drop_graph()
            if self._ring is None:
                self._ring = [p.detach().clone() for p in model.prevs]
            else:
                for ring, p in zip(self._ring, model.prevs):
                    ring.copy_(p)
            model.prevs = self._ring
        self.t = 0
        return self._wrap(out, out[0])

    def _hold_references(self, ref_labels, ref_images):
        """frame 0 with keep_references / inputs_u8: the sequence's references (converted from uint8 where they arrive so) into
        static buffers - allocated for new shapes, rewritten in place otherwise"""
        refs = (ref_labels, ref_images)
        if self._ref_in is None:
            # (_in is None here as well: the two are dropped together, _drop_buffers)
            self._ref_in = [ops.image_from_u8(t) if self.inputs_u8 else t.detach().clone() for t in refs]
        else:
            for dst, src in zip(self._ref_in, refs):
                if self.inputs_u8:
                    ops.image_from_u8(src, out=dst)
                else:
                    dst.copy_(src)
        return self._ref_in

    def _keep_sequence(self):
        """generated weights and the deepest reference feature of this sequence into the session's static buffers"""
        netG = self.model.netG
        cw, x = netG._cached_weights, netG._cached_x
        old = _flat_tensors(self._static_w)
        new = _flat_tensors(cw)
        if (self._static_w is None or len(old) != len(new) or any(a.shape != b.shape for a, b in zip(old, new)) or
                self._static_x.shape != x.shape):
            if self._graph is not None:
                self._drop_graph()
            memo = {}

            def clone(t):
                if id(t) not in memo:
                    c = t.detach().clone()
                    c._fsv_frozen = self.frozen
                    memo[id(t)] = c
                return memo[id(t)]
            self._static_w = _map_tensors(cw, clone)
            self._static_x = x.detach().clone()
        else:
            done = set()
            for dst, src in zip(old, new):
                if id(dst) not in done:
                    dst.copy_(src)
                    done.add(id(dst))
            self._static_x.copy_(x)
            self.frozen.refill()
        if self._graph is not None and not self._graph_has_x:
            self._drop_graph()                   # captured while the reference feature was recomputed per frame (refreeze)
        netG._cached_weights = self._static_w
        netG._cached_x = self._static_x
        netG._frozen_x = self._static_x

    # ------------------------------------------------------------------------------------------------ steady frames
    def _body(self):
        """one frame t >= 1 on the static buffers: Vid2VidModel.inference itself, then the ring advanced in place"""
        model = self.model
        model.prevs, model.t = self._ring, self.t
        # the generator opens its own statistics pass (conv.stats_pass): make it the outermost one even under Vid2VidModel.forward's,
        # so that the arena's zeroing is part of the captured frame whichever way the session is called
        arena = conv.stats_arena(self._in[0].device) if conv.stats_enabled() else None
        depth = arena.depth if arena is not None else 0
        if arena is not None:
            arena.depth = 0
        try:
            out = model.inference(*self._in)
        finally:
            if arena is not None:
                arena.depth = depth
        with torch.no_grad():
            for ring, new in zip(self._ring, model.prevs):
                ring.copy_(new)
            u8 = ops.image_u8(out[0]) if self.frames_u8 else None
        model.prevs = self._ring
        self._out = (out, u8)

    def _capture(self):
        dev = self._in[0].device
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph(keep_graph=True) if self.keep_graph else torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._body()
        self._graph, self._graph_has_x = g, self.model.netG._frozen_x is not None
        self.n_captures += 1

    def _capture_failed(self, ex):
        self._graph, self._eager_only = None, True
        self.capture_failures.append((self._sig, str(ex).split('\n')[0][:200]))
        try:
            torch.cuda.synchronize(self._in[0].device)
        except Exception:                        # noqa: BLE001
            pass

    def _steady_frame(self, tgt_label, ref_labels, ref_images):
        ins = (tgt_label, ref_labels, ref_images)
        if self._signature(ins) != self._sig:
            raise RuntimeError("the frame's tensors changed shape, dtype or device inside a sequence; call reset() first")
        held = self._kept is not None and self._ref_in is not None      # the references were read at frame 0
        if self._in is None:
            tgt = ops.image_from_u8(tgt_label) if self.inputs_u8 else tgt_label.detach().clone()
            if held:
                self._in = [tgt] + list(self._ref_in)
            elif self.inputs_u8:
                self._in = [tgt] + list(self._ref_in)
                for dst, src in zip(self._in[1:], ins[1:]):
                    ops.image_from_u8(src, out=dst)
            else:
                self._in = [tgt] + [t.detach().clone() for t in ins[1:]]
        else:
            for dst, src in zip(self._in, ins[:1] if held else ins):
                if self.inputs_u8:
                    ops.image_from_u8(src, out=dst)
                else:
                    dst.copy_(src, non_blocking=True)
        self._steady += 1
        if self._emulated or self._eager_only or self._steady <= self.warmup:
            if not self._emulated and self._steady == 1:
                # warm-up on a side stream so that allocations made now do not end up in the capture's private pool
                s = torch.cuda.Stream(self._in[0].device)
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    self._body()
                torch.cuda.current_stream().wait_stream(s)
            else:
                self._body()
        elif self._graph is None:
            try:
                self._capture()
            except Exception as ex:              # noqa: BLE001 - a capture fault must never cost the caller its frame
                self._capture_failed(ex)
                self._body()
            else:
                self._graph.replay()
        else:
            self._graph.replay()
        self.t += 1
        self.model.prevs, self.model.t = self._ring, self.t
        out, u8 = self._out
        return self._wrap(out, None, u8)

    def _wrap(self, out, fake=None, u8=None):
        res = FrameOutputs(out)
        if self.frames_u8:
            res.image_u8 = u8 if u8 is not None else ops.image_u8(fake)
        return res

    def __call__(self, tgt_label, ref_labels, ref_images):
        """one frame; the tensors of a replayed frame are the graph's static outputs: consume (or clone) them before the next call"""
        if self.model.training:
            raise RuntimeError("the model went back to train() mode under an InferenceSession; close() it first")
        if self.frozen is None:
            raise RuntimeError("this InferenceSession is closed")
        if self.t is None or getattr(self.model, 'prevs', None) is None:
            return self._frame0(tgt_label, ref_labels, ref_images)
        return self._steady_frame(tgt_label, ref_labels, ref_images)
