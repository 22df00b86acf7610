"""Generator / discriminator networks of the few-shot-vid2vid hot path on the HIP operators in ops.py.

Same operator surface and - deliberately - the same ``state_dict`` key layout as the reference's
``models.networks`` (generator.py, architecture.py, normalization.py, discriminator.py), so that reference
checkpoints load unchanged and these classes can be patched into the reference's train.py loop
(see INTEGRATION.md).  The bodies are new: every convolution, normalisation, SPADE modulation, up-sampling and
warp goes through the gfx950 kernels, activations stay channels-last between layers, and element-wise chains
of the reference are folded into kernel epilogues (bias+LeakyReLU, tanh, sigmoid, flow scale, residual add,
BN+LeakyReLU, SPADE denorm+modulate+LeakyReLU).
"""
import contextlib
import math
import os
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops, streams
from .conv import ACT_LRELU, ACT_NONE, ACT_SIGMOID, ACT_TANH, empty_nhwc, to_nhwc


# ------------------------------------------------------------------------------------------------ parameter holders
class _SpectralMixin:
    def _init_spectral(self, weight):
        rows = weight.shape[0]
        cols = weight.numel() // rows
        self.weight_orig = nn.Parameter(weight)
        self.register_buffer('weight_u', F.normalize(torch.randn(rows), dim=0, eps=1e-12))
        self.register_buffer('weight_v', F.normalize(torch.randn(cols), dim=0, eps=1e-12))

    _sig_cached = None
    _sig_frozen = None                   # (sigma, 1 / sigma) taken once by an infer.InferenceSession: eval() only, until it refreezes

    def _sn(self):
        cached = self._sig_cached        # (sigma pair, u snapshot, v snapshot) from the network-level batched pass
        if cached is not None:
            self._sig_cached = None
            return (cached[0], cached[1], cached[2], True)
        if self._sig_frozen is not None and not self.training:
            return (self._sig_frozen, self.weight_u, self.weight_v, False)
        sig = ops.SpectralState.update(self.weight_orig, self.weight_u, self.weight_v, self.training)
        return (sig, self.weight_u, self.weight_v, False)


class Conv2d(nn.Module, _SpectralMixin):
    """nn.Conv2d (+ optional torch.nn.utils.spectral_norm) with a fused epilogue."""

    def __init__(self, cin, cout, k, stride=1, padding=0, bias=True, spectral=False):
        super().__init__()
        self.stride, self.padding, self.spectral = stride, padding, spectral
        w = torch.empty(cout, cin, k, k)
        if spectral:
            nn.init.kaiming_uniform_(w, a=math.sqrt(5))       # what survives the reference's init
            self._init_spectral(w)
        else:
            nn.init.xavier_normal_(w, gain=0.02)              # init_type 'xavier', init_variance 0.02
            self.weight = nn.Parameter(w)
        self.bias = nn.Parameter(torch.zeros(cout)) if bias else None

    # infer.InferenceSession(fold_norms=True): (shift vector t, the eval-mode BatchNorm that reads this layer's output and nothing
    # else).  The frozen layout of the weight then carries gamma * rstd / sigma in its columns, and this launch is
    # LeakyReLU(conv + t): the BatchNorm finds its own mark on the tensor and hands it on.
    _fsv_fold = None

    def forward(self, x, act=ACT_NONE, res=None, scale=1.0, stats=0, up=False):
        """stats: 1 / -1 when a BatchNorm / InstanceNorm consumes the output next (ops.conv2d stats_groups: the statistics then
        come out of this launch's epilogue instead of a read pass over the output).  up: the convolution of the nearest x2
        up-sampling of x (nn.Upsample in front of this layer in the reference: ops.conv2d folds it into the gather)"""
        fold = self._fsv_fold
        if fold is not None and not self.training and not torch.is_grad_enabled():
            if act != ACT_NONE or res is not None or scale != 1.0:
                raise ValueError("a convolution with a folded BatchNorm is called with an epilogue of its own")
            y = ops.conv2d(x, self.weight_orig if self.spectral else self.weight, fold[0], self.stride, self.padding, ACT_LRELU,
                           1.0, None, None, 0, up)
            y._fsv_folded_bn = fold[1]
            return y
        if self.spectral:
            return ops.conv2d(x, self.weight_orig, self.bias, self.stride, self.padding, act, scale, res, self._sn(), stats, up)
        return ops.conv2d(x, self.weight, self.bias, self.stride, self.padding, act, scale, res, None, stats, up)


class Linear(nn.Module, _SpectralMixin):
    def __init__(self, cin, cout, spectral=True):
        super().__init__()
        w = torch.empty(cout, cin)
        nn.init.kaiming_uniform_(w, a=math.sqrt(5))
        self.spectral = spectral
        if spectral:
            self._init_spectral(w)
        else:
            self.weight = nn.Parameter(w)
        self.bias = nn.Parameter(torch.zeros(cout))

    def forward(self, x, act=ACT_NONE):
        if self.spectral:
            return ops.linear(x, self.weight_orig, self.bias, act, self._sn())
        return ops.linear(x, self.weight, self.bias, act, None)


class BatchNorm(nn.Module):
    """Train-mode BatchNorm2d statistics holder (apex SyncBatchNorm in one process)."""

    def __init__(self, c, affine=True):
        super().__init__()
        self.affine = affine
        if affine:
            self.weight = nn.Parameter(torch.ones(c))
            self.bias = nn.Parameter(torch.zeros(c))
        self.register_buffer('running_mean', torch.zeros(c))
        self.register_buffer('running_var', torch.ones(c))
        self.register_buffer('num_batches_tracked', torch.tensor(0, dtype=torch.long))
        # the counter does not enter the maths (momentum is fixed); it is kept on the host and folded into the buffer
        # when a checkpoint is taken, so that no extra kernel is launched per normalisation call
        self._pending = 0
        self.register_state_dict_pre_hook(BatchNorm._flush)

    @staticmethod
    def _flush(module, prefix, keep_vars):
        if module._pending:
            module.num_batches_tracked += module._pending
            module._pending = 0

    def note_forward(self):
        if self.training:
            self._pending += 1

    MOMENTUM = 0.1

    def stats_hint(self, training):
        # (the hint only pays when the consumer reduces batch statistics: eval-mode BatchNorm takes its running buffers)
        return 1 if training else 0

    def forward(self, x, act=ACT_NONE):
        if getattr(x, '_fsv_folded_bn', None) is self:          # (Conv2d._fsv_fold: the producer already applied this layer)
            if act != ACT_LRELU or self.training:
                raise ValueError("a folded BatchNorm is LeakyReLU(eval-mode affine norm) only")
            return x
        self.note_forward()
        return ops.norm_act(x, self.weight if self.affine else None, self.bias if self.affine else None,
                            self.running_mean, self.running_var, instance=False, eps=1e-5, momentum=BatchNorm.MOMENTUM, act=act,
                            training=self.training)


class InstanceNorm(nn.Module):
    """nn.InstanceNorm2d without running buffers: the discriminator's and get_nonspade_norm_layer's (affine=True, eps=0.1), the
    parameter-free ones of SPADE (affine=False, eps=0.1) and of generalNorm (affine=False, torch's eps).  The same in eval()."""

    def __init__(self, c, affine=True, eps=0.1):
        super().__init__()
        self.affine, self.eps = affine, eps
        if affine:
            self.weight = nn.Parameter(torch.ones(c))
            self.bias = nn.Parameter(torch.zeros(c))

    def stats_hint(self, training):
        return -1

    def forward(self, x, act=ACT_NONE):
        return ops.norm_act(x, self.weight if self.affine else None, self.bias if self.affine else None, None, None, instance=True,
                            eps=self.eps, act=act, training=True)


NORMS_G = ('spectralspadesyncbatch', 'spectralspadebatch', 'spectralspadeinstance')
NORMS_F = ('spectralsyncbatch', 'spectralbatch', 'spectralinstance', 'spectralnone')


def norm_kind(norm, spade=False):
    """'batch' / 'instance' / 'none' of a --norm_G (spade=True: generator.py:32, only the SPADE main branch is built here) or of a
    --norm_F / norm_ref string (normalization.py:64-84)"""
    if spade:
        if norm not in NORMS_G:
            raise NotImplementedError("norm_G = %r: only %s" % (norm, ', '.join(NORMS_G)))
        norm = norm.replace('spade', '')
    if norm not in NORMS_F:
        raise ValueError('normalization layer %s is not recognized' % (norm[len('spectral'):] if str(norm).startswith('spectral')
                                                                       else norm,))
    sub = norm[len('spectral'):]
    return 'batch' if 'batch' in sub else sub


def make_norm(norm, c, role):
    """The normalisation module a norm string stands for, by where it sits:
      'spade'  SPADE.norm (normalization.py:32-35): parameter-free; InstanceNorm2d(eps=0.1) or the batch norm
      'plain'  generalNorm's NormalNorm (architecture.py:40-55: SPADEConv2d.bn, the bn_* of a block without SPADE): torch's defaults -
               affine BatchNorm, or InstanceNorm2d(affine=False, eps=1e-5)
      'layer'  get_nonspade_norm_layer (normalization.py:77-84): affine BatchNorm / InstanceNorm2d(affine=True, eps=0.1); None for
               'spectralnone' (the convolution then keeps its bias and stands alone in its slot)"""
    kind = norm_kind(norm, spade=(role == 'spade'))
    if role == 'spade':
        return InstanceNorm(c, affine=False, eps=0.1) if kind == 'instance' else BatchNorm(c, affine=False)
    if role == 'plain':
        if kind == 'none':
            # (the reference fails here too: generalNorm derives NormalNorm from None - `--norm_F spectralnone` needs --n_blocks_F 0)
            raise TypeError("norm %r names no normalisation class for a residual block (architecture.py:40-55: the reference raises "
                            "'NoneType takes no arguments'); use --n_blocks_F 0 with it" % (norm,))
        return InstanceNorm(c, affine=False, eps=1e-5) if kind == 'instance' else BatchNorm(c, affine=True)
    if kind == 'none':
        return None
    return InstanceNorm(c, affine=True, eps=0.1) if kind == 'instance' else BatchNorm(c, affine=True)


class _Slot(nn.Module):
    """Parameter-free placeholder that keeps nn.Sequential-style numeric keys aligned with the reference."""

    def forward(self, x):
        return x


def _seq(*mods):
    return nn.ModuleList(list(mods))


# ------------------------------------------------------------------------------------------------ building blocks
class SPADEConv2d(nn.Module):
    """conv3x3(SN) -> norm -> LeakyReLU  (reference architecture.py:57-69): affine BatchNorm for norm='spectralsyncbatch' /
    'spectralbatch', nn.InstanceNorm2d with torch's defaults (no parameters, no buffers) for 'spectralinstance'."""

    def __init__(self, fin, fout, stride=1, norm='spectralsyncbatch'):
        super().__init__()
        self.conv = Conv2d(fin, fout, 3, stride=stride, padding=1, spectral=True)
        self.bn = make_norm(norm, fout, 'plain')

    def forward(self, x):
        return self.bn(self.conv(x, stats=self.bn.stats_hint(self.training)), act=ACT_LRELU)


class SPADE(nn.Module):
    """Reference normalization.py:18-52 (ks = 1 or 3): param-free BatchNorm (or, for a norm with 'instance', InstanceNorm2d with
    eps = 0.1) + sequential (1+gamma)*x+beta per map."""

    def __init__(self, norm_nc, hidden_nc, params_free=False, ks=1, norm='spectralspadesyncbatch'):
        super().__init__()
        if not isinstance(hidden_nc, list):
            hidden_nc = [hidden_nc]
        self.n_hidden = len(hidden_nc)
        self.params_free = params_free
        self.ks = ks
        for i, nh in enumerate(hidden_nc):
            if not params_free or i != 0:
                s = str(i + 1) if i > 0 else ''
                setattr(self, 'mlp_gamma%s' % s, Conv2d(nh, norm_nc, ks, padding=ks // 2))
                setattr(self, 'mlp_beta%s' % s, Conv2d(nh, norm_nc, ks, padding=ks // 2))
        self.norm = make_norm(norm, norm_nc, 'spade')
        self.instance = isinstance(self.norm, InstanceNorm)
        self.norm_nc = norm_nc

    def stats_hint(self, training):
        return self.norm.stats_hint(training)

    def forward(self, x, maps, weights=None, act=ACT_NONE, up=False):
        if not isinstance(maps, list):
            maps = [maps]
        use_maps, use_w = [], []
        for i, m in enumerate(maps):
            if m is None:
                continue
            if weights is None or i != 0:
                s = str(i + 1) if i > 0 else ''
                g, b = getattr(self, 'mlp_gamma%s' % s), getattr(self, 'mlp_beta%s' % s)
                use_w.append((g.weight, b.weight, g.bias, b.bias))
            else:
                # generated weights of map 0: the reference indexes weights[0][j] / weights[1][j], i.e. the weight
                # tensors only - the generated biases never reach batch_conv (normalization.py:48-50)
                wg, wb = weights[0][0], weights[1][0]
                zb = getattr(self, '_zero_bias', None)
                if zb is None or zb.shape[0] != wg.shape[0] or zb.device != wg.device:
                    zb = self._zero_bias = streams.shared(
                        lambda: torch.zeros(wg.shape[0], self.norm_nc, dtype=wg.dtype, device=wg.device))
                use_w.append((wg, wb, zb, zb))
            use_maps.append(m)
        if self.instance:
            return ops.spade_mod(x, use_maps, use_w, None, None, act=act, training=True, eps=self.norm.eps, up=up, instance=True)
        self.norm.note_forward()
        return ops.spade_mod(x, use_maps, use_w, self.norm.running_mean, self.norm.running_var, act=act, training=self.training, up=up)


class AdaptiveConv2d(nn.Module):
    """architecture.py:31-35 (--adaptive_conv): a convolution without parameters of its own - weight [B, Cout, Cin, k, k] and bias
    [B, Cout] come from the weight generators, one set per sample (ops.batch_conv, padding k // 2)"""

    def forward(self, x, act=ACT_NONE, res=None, stats=0, wb=None):
        # (stats: the BatchNorm-statistics epilogue is a shared-weight launch's; the normalisation that follows reduces itself)
        if wb is None:
            raise ValueError("a parameter-free convolution needs generated weights (conv_weights)")
        return ops.batch_conv(x, wb[0], wb[1], act=act, res=res)


class SPADEResnetBlock(nn.Module):
    """Reference architecture.py:71-108 (SPADE or plain-BatchNorm flavour).  conv_params_free (--adaptive_conv): conv_0, conv_1 and
    conv_s own no parameters and no spectral norm; forward() takes their per-sample [weight, bias] pairs as `conv_weights`."""

    def __init__(self, fin, fout, hidden_nc=0, spade=True, norm_params_free=False, spade_ks=1, conv_params_free=False, norm=None):
        super().__init__()
        if norm is None:
            norm = 'spectralspadesyncbatch' if spade else 'spectralsyncbatch'
        self.spade_ks = spade_ks
        fhidden = min(fin, fout)
        self.learned_shortcut = fin != fout
        self.spade = spade
        self.conv_params_free = conv_params_free
        if conv_params_free:
            self.conv_0, self.conv_1 = AdaptiveConv2d(), AdaptiveConv2d()
            if self.learned_shortcut:
                self.conv_s = AdaptiveConv2d()          # (its generated form HAS a bias: generator.py:288)
        else:
            self.conv_0 = Conv2d(fin, fhidden, 3, padding=1, spectral=True)
            self.conv_1 = Conv2d(fhidden, fout, 3, padding=1, spectral=True)
            if self.learned_shortcut:
                self.conv_s = Conv2d(fin, fout, 1, bias=False, spectral=True)
        if spade:
            self.bn_0 = SPADE(fin, hidden_nc, norm_params_free, spade_ks, norm)
            self.bn_1 = SPADE(fhidden, hidden_nc, norm_params_free, spade_ks, norm)
            if self.learned_shortcut:
                self.bn_s = SPADE(fin, hidden_nc, norm_params_free, spade_ks, norm)
        else:
            self.bn_0 = make_norm(norm, fin, 'plain')
            self.bn_1 = make_norm(norm, fhidden, 'plain')
            if self.learned_shortcut:
                self.bn_s = make_norm(norm, fin, 'plain')

    def _conv(self, name, x, wb, **kw):
        m = getattr(self, name)
        return m(x, wb=wb, **kw) if self.conv_params_free else m(x, **kw)

    def forward(self, x, label=None, norm_weights=None, up=False, feeds_norm=True, conv_weights=None):
        """up=True: x is the block input BEFORE the nearest x2 up-sampling of generator.py:124.  With a learned shortcut
        the up-sampled tensor is consumed only by bn_0 and bn_s, which read x through the up-sampling index (ops.spade_mod
        up=True) - it is never written; otherwise it is materialised here.  conv_weights: [[weight, bias]] x 3 for conv_0, conv_1,
        conv_s of a conv_params_free block.  The fused SPADE -> convolution launches are written for shared weights: handed a
        per-sample convolution they decline (ops._spade_conv_s_fits / _spade_conv3_fits) and the held-back modulation runs as its
        own launch."""
        nw = norm_weights if norm_weights else [None] * 3
        cw = conv_weights if conv_weights else [None] * 3
        fold = (up and self.spade and self.learned_shortcut and x.shape[1] % 16 == 0 and
                ops.spade_can_fold_upsample(instance=self.bn_0.instance))
        if up and not fold:
            x = ops.upsample2x(x)
        if self.spade:
            # the fused SPADE launches (bn_s -> conv_s, actvn(bn) -> conv3x3) are 1x1-only: a 3x3 SPADE (--spade_ks 3) declines
            # them here and runs as its own launch (csrc/spade_k3.hip) followed by the gather-GEMM convolution
            k1 = self.spade_ks == 1
            conv3 = k1 and ops.spade_conv3_enabled()
            if self.learned_shortcut:
                # bn_s -> conv_s as ONE kernel where csrc/spade_conv.hip covers the widths (ops.spade_into_conv)
                with (ops.spade_into_conv() if k1 else contextlib.nullcontext()):
                    x_s = self._conv('conv_s', self.bn_s(x, label, nw[2], act=ACT_NONE, up=fold), cw[2])
            else:
                x_s = x
            h0 = None if conv3 else self.bn_0(x, label, nw[0], act=ACT_LRELU, up=fold)
            # conv_0 feeds bn_1, conv_1 (+ shortcut) the next block's bn_0 / bn_s: BatchNorm statistics from their epilogues
            # (in training mode only: eval-mode BatchNorm takes its running buffers and would leave the partials unused; a next
            # block that materialises the up-sampling - up and not fold - reduces over the up-sampled tensor itself)
            # (an instance norm reduces per sample in eval() too: -1)
            hint = self.bn_1.stats_hint(self.training)
            if conv3:
                # round 6, opt-in (FSV_SPADE_CONV3=1): actvn(bn_*) -> 3x3 convolution as ONE kernel where csrc/spade_conv3.hip covers
                # the widths (the modulated tensor stays in LDS); anything else falls through to the two launches
                with ops.spade_into_conv(conv3=True):
                    dx = self._conv('conv_0', self.bn_0(x, label, nw[0], act=ACT_LRELU, up=fold), cw[0], stats=hint)
                with ops.spade_into_conv(conv3=True):
                    return self._conv('conv_1', self.bn_1(dx, label, nw[1], act=ACT_LRELU), cw[1], res=x_s,
                                      stats=hint if feeds_norm else 0)
            dx = self._conv('conv_0', h0, cw[0], stats=hint)
            return self._conv('conv_1', self.bn_1(dx, label, nw[1], act=ACT_LRELU), cw[1], res=x_s, stats=hint if feeds_norm else 0)
        hint = self.bn_1.stats_hint(self.training)
        x_s = self._conv('conv_s', self.bn_s(x), cw[2]) if self.learned_shortcut else x
        dx = self._conv('conv_0', self.bn_0(x, act=ACT_LRELU), cw[0], stats=hint)
        return self._conv('conv_1', self.bn_1(dx, act=ACT_LRELU), cw[1], res=x_s, stats=hint if feeds_norm else 0)


def _decode_early():
    import os
    return streams.ENABLED and os.environ.get('FSV_DECODE_EARLY', '1') == '1'


def spectral_layers(module):
    """every spectral-normalised Conv2d / Linear below `module`, each once, in registration order"""
    seen, out = set(), []
    for m in module.modules():
        if getattr(m, 'spectral', False) and id(m) not in seen:
            seen.add(id(m))
            out.append(m)
    return out


def _channels(nf, n, cap=1024):
    return [min(cap, nf * (2 ** i)) for i in range(n)]


class LabelEmbedder(nn.Module):
    """Reference generator.py:506-572: encoder(-decoder / U-Net) producing one SPADE map per generator level."""

    def __init__(self, opt, input_nc, netS, params_free_layers=0):
        super().__init__()
        # generator.py:510 builds get_nonspade_norm_layer(opt, opt.norm_F) and never applies it: every convolution here is bare
        # under every --norm_F; the string is only held to the accepted set
        norm_kind(getattr(opt, 'norm_F', 'spectralsyncbatch'))
        nf = opt.ngf
        self.unet = 'unet' in netS
        self.decode = 'decoder' in netS or self.unet
        self.n = n = opt.n_downsample_G
        self.embed_ks = getattr(opt, 'embed_ks', 1)
        self.params_free_layers = params_free_layers if params_free_layers != -1 else n
        ch = _channels(nf, n + 1)
        self.conv_first = _seq(Conv2d(input_nc, nf, 3, padding=1), _Slot())
        for i in range(n):
            if i >= params_free_layers or 'decoder' in netS:
                setattr(self, 'down_%d' % i, _seq(Conv2d(ch[i], ch[i + 1], 3, stride=2, padding=1), _Slot()))
        if self.decode:
            for i in reversed(range(n)):
                ch_i = ch[i + 1] * (2 if self.unet and i != n - 1 else 1)
                if i >= params_free_layers:
                    setattr(self, 'up_%d' % i, _seq(_Slot(), Conv2d(ch_i, ch[i], 3, padding=1), _Slot()))

    def forward(self, x, weights=None):
        return self.decode_maps(self.encode_maps(x), weights)

    def encode_maps(self, x):
        """the part that needs no generated weights: the encoder and the decoder levels with parameters of their own (it
        runs next to the reference encoders that produce those weights, see FewShotGenerator.flow_branch)"""
        if x is None:
            return None
        n = self.n
        out = [self.conv_first[0](x, act=ACT_LRELU)]
        for i in range(n):
            if i >= self.params_free_layers or self.decode:
                out.append(getattr(self, 'down_%d' % i)[0](out[-1], act=ACT_LRELU))
            else:
                raise NotImplementedError("adaptive strided embedding convs are not used by any shipped config")
        if not self.decode:
            return out
        skips = out
        if not self.unet:
            out = [out[-1]]
        out = list(out)
        for i in reversed(range(n)):
            if i < self.params_free_layers:
                break
            out.append(self._up(i, out[-1], skips, None))
        return out, skips

    def _up(self, i, cur, skips, weights):
        if self.unet and i != self.n - 1:
            cur = ops.cat_channels([cur, skips[i + 1]])
        if i >= self.params_free_layers:
            return getattr(self, 'up_%d' % i)[1](cur, act=ACT_LRELU, up=True)      # generator.py:559-563: Upsample -> conv3x3
        w, b = weights[i]
        if self.embed_ks != 1:
            # --embed_ks 3 (generator.py:566-568): nearest x2 up-sampling, then the per-sample 3x3 convolution (padding 1), LeakyReLU
            return ops.batch_conv(ops.upsample2x(cur), w, b, act=ACT_LRELU)
        # a 1x1 convolution commutes with nearest up-sampling: run the generated-weight conv on the quarter-size
        # tensor, then up-sample (bit-identical, 4x fewer MACs and bytes)
        return ops.upsample2x(ops.batch_conv(cur, w, b, act=ACT_LRELU))

    def decode_maps(self, state, weights=None):
        if state is None or not self.decode:
            return state
        out, skips = state
        out = list(out)
        for i in reversed(range(min(self.n, self.params_free_layers))):
            out.append(self._up(i, out[-1], skips, weights))
        if self.unet:
            out = out[self.n:]
        return out[::-1]


class FlowGenerator(nn.Module):
    """Reference generator.py:456-504."""

    def __init__(self, opt, n_frames_G):
        super().__init__()
        input_nc = (opt.label_nc if opt.label_nc != 0 else opt.input_nc) * n_frames_G + opt.output_nc * (n_frames_G - 1)
        nf, nd = opt.nff, opt.n_downsample_F
        self.nd = nd
        self.flow_multiplier = opt.flow_multiplier
        ch = _channels(nf, nd + 1)

        norm = getattr(opt, 'norm_F', 'spectralsyncbatch')

        def normed(cin, cout, stride=1):
            # get_nonspade_norm_layer (normalization.py:62-86): Sequential(sn(conv without bias), norm) - or, for 'spectralnone', the
            # spectral convolution itself, bias kept, in the same slot
            layer = make_norm(norm, cout, 'layer')
            if layer is None:
                return Conv2d(cin, cout, 3, stride=stride, padding=1, bias=True, spectral=True)
            return _seq(Conv2d(cin, cout, 3, stride=stride, padding=1, bias=False, spectral=True), layer)
        down = [normed(input_nc, nf), _Slot()]
        for i in range(nd):
            down += [normed(ch[i], ch[i + 1], 2), _Slot()]
        self.down_flow = _seq(*down)
        self.res_flow = _seq(*[SPADEResnetBlock(ch[nd], ch[nd], spade=False, norm=norm) for _ in range(opt.n_blocks_F)])
        up = []
        for i in reversed(range(nd)):
            up += [_Slot(), normed(ch[i + 1], ch[i]), _Slot()]
        self.up_flow = _seq(*up)
        self.conv_flow = _seq(Conv2d(nf, 2, 3, padding=1))
        self.conv_mask = _seq(Conv2d(nf, 1, 3, padding=1), _Slot())

    def _normed(self, layer, x, up=False):
        if isinstance(layer, Conv2d):           # 'spectralnone': convolution (+ bias) -> LeakyReLU
            return layer(x, act=ACT_LRELU, up=up)
        conv, bn = layer
        return bn(conv(x, stats=bn.stats_hint(self.training), up=up), act=ACT_LRELU)

    def forward(self, label, label_prev, img_prev, for_ref=False):
        x = ops.cat_channels([label, label_prev, img_prev])
        for k in range(0, 2 * (self.nd + 1), 2):
            x = self._normed(self.down_flow[k], x)
        for k, blk in enumerate(self.res_flow):
            x = blk(x, feeds_norm=k + 1 < len(self.res_flow))
        for k in range(1, 3 * self.nd, 3):
            x = self._normed(self.up_flow[k], x, up=True)           # generator.py:489-493: Upsample -> conv
        flow = self.conv_flow[0](x, scale=float(self.flow_multiplier))
        mask = self.conv_mask[0](x, act=ACT_SIGMOID)
        return flow, mask


def pick_ref(refs, ref_idx):
    """base_network.py:40-47: the reference with the largest attention mass per sample (the first one for n_shot == 1)"""
    if ref_idx is None:
        return refs[:, 0]
    return refs[torch.arange(refs.shape[0], device=refs.device), ref_idx.long()]


# ------------------------------------------------------------------------------------------------ attention in query bands
# The attention of n_shot > 1 (generator.py:298-316) materialises energy / attention [b, n*hw, h, w] in fp32; one gather-GEMM launch
# reads at most ATTN_LAUNCH_MAX_BYTES of input, all samples of the launch together (include/fsv2v.h, csrc/conv_igemm.h
# FSV_BUF_MAX_BYTES).  The softmax is over the n*hw key positions of each query pixel, so query pixels are independent: the three
# launches (energy GEMM, softmax, weighted sums) run per BAND of query positions - a range of whole samples, or a range of rows of
# the h x w query grid of one sample; either is one dense piece of channels-last memory - against the same key / reference operands.
ATTN_LAUNCH_MAX_BYTES = 1 << 31


def attention_band_plan(b, n, hw, h, w):
    """-> None: one launch covers the attention and FSV_ATTN_BAND_MB is unset (the unbanded code runs, launch for launch), else the
    bands [(s0, s1, r0, r1)]: samples s0 .. s1 - 1, rows r0 .. r1 - 1.  The largest bands whose energy / attention slice stays at or
    under min(ATTN_LAUNCH_MAX_BYTES, FSV_ATTN_BAND_MB * 2^20): whole samples while one sample fits (the per-sample launches count the
    bytes of all their samples), rows of one sample otherwise - the last band of a sample (of the batch) takes the remainder.
    FSV_ATTN_BAND_MB (a number, fractions allowed; read per call): for tests and A/B runs."""
    cap = ATTN_LAUNCH_MAX_BYTES
    forced = os.environ.get('FSV_ATTN_BAND_MB', '')
    if forced:
        mb = float(forced)
        if not mb > 0:
            raise ValueError("FSV_ATTN_BAND_MB=%r: a positive number of MiB expected" % forced)
        cap = min(cap, int(mb * (1 << 20)))
    row_bytes = n * hw * w * 4
    sample_bytes = row_bytes * h
    if not forced and b * sample_bytes <= cap:
        return None
    if sample_bytes <= cap:
        per = min(b, cap // sample_bytes)
        return [(s, min(b, s + per), 0, h) for s in range(0, b, per)]
    rows = cap // row_bytes
    if rows < 1:
        raise ValueError("attention: one row of %d query positions against %d x %d key positions is %d bytes, over the %d of one band"
                         % (w, n, hw, row_bytes, cap))
    return [(s, s + 1, r, min(h, r + rows)) for s in range(b) for r in range(0, h, rows)]


def _switch01(name):
    """the 0 / 1 environment switch `name` (default 0; read per call)"""
    v = os.environ.get(name, '')
    if not v:
        return False
    try:
        f = float(v)
    except ValueError:
        f = -1.0
    if f not in (0.0, 1.0):
        raise ValueError("%s=%r: 0 or 1 expected" % (name, v))
    return f == 1.0


def attention_fused_switch(net=None):
    """FSV_ATTN_FUSED (0 / 1, default 0; read per call), or a network an InferenceSession(fused_attention=True) marked: the attention
    of n_shot > 1 as one streaming launch - where autograd is off and ops.attention_fused serves the shape; ignored otherwise"""
    marked = net is not None and net.__dict__.get('_attn_fused', False)
    return not torch.is_grad_enabled() and (marked or _switch01('FSV_ATTN_FUSED'))


def attention_half_switch(net):
    """FSV_ATTN_FUSED_HALF (0 / 1, default 0; read per call), or a network an InferenceSession(fused_attention='half') marked: the
    attention of n_shot > 1 as the streaming launch on the f16 matrix cores (ops.attention_fused_half) - an INFERENCE path: where
    autograd is off, the generator is in eval() and the kernel serves the shape; ignored otherwise (a training pass never takes it,
    nor does the D step's generator pass: the generator is in train() there).  Independent of FSV_ATTN_FUSED; where both are set and
    the half kernel serves the shape, half wins."""
    if torch.is_grad_enabled() or net.training:
        return False
    return bool(net.__dict__.get('_attn_half', False)) or _switch01('FSV_ATTN_FUSED_HALF')


def attention_fused_grad_switch():
    """FSV_ATTN_FUSED_GRAD (0 / 1, default 0; read per call): the attention of n_shot > 1 of a DIFFERENTIABLE pass as the streaming
    forward launch plus the streaming backward kernels (ops.attention_fused_grad) - where autograd is on and the backward serves the
    shape; ignored otherwise.  Independent of FSV_ATTN_FUSED, which speaks for the no-grad passes only."""
    return torch.is_grad_enabled() and _switch01('FSV_ATTN_FUSED_GRAD')


def _kmat(key, b, n, hw):
    """key features [b*n, c, h, w] as the per-sample 1x1 weights [b, n*hw, c, 1, 1] of the energy GEMM"""
    c = key.shape[1]
    return key.reshape(b, n, c, hw).permute(0, 1, 3, 2).reshape(b, n * hw, c, 1, 1)


def _xmat(x, b, n, hw):
    """reference features [b*n, c, h, w] as the per-sample 1x1 weights [b, c, n*hw, 1, 1] of the weighted-sum GEMM (a session's kept
    operand is in that arrangement already)"""
    c = x.shape[1]
    return x if x.dim() == 5 else x.reshape(b, n, c, hw).permute(0, 2, 1, 3).reshape(b, c, n * hw, 1, 1)


class _Attention:
    """the attention of one pass, one of the kinds below.  attend(values, want_mass) -> [attended map per value map] is the only
    place a kind's launches are issued: want_mass on the pass's first call, which forms the attention and mass[b, h, w, n] (the sum
    over each reference's hw key positions: atn_vis, ref_idx); a later call, for a map the first was not told of, re-uses what the
    kind kept.  operands(): the (name, tensor) pairs of the last call, for a session's sink (infer.KeptReferences.keep).  second:
    (the tensor, its attended feature) of a map that was announced and rode in the first call.  handle(): what is handed out as `atn`."""
    KEY, VALUE = 'kmat', 'xmat%d'

    def __init__(self, b, n, hw, h, w):
        self.b, self.n, self.hw, self.h, self.w = b, n, hw, h, w
        self.mass = self.second = None
        self._offer = []

    def atn_vis(self):
        return self.mass.permute(0, 3, 1, 2)[-1:, 0:1]

    def ref_idx(self):
        return torch.argmax(self.mass.sum((1, 2)), dim=1)

    def operands(self):
        return self._offer

    def handle(self):
        return self

    def _offers(self, first, key, values):
        """the first call offers the key side and its maps as 0, 1; a later call its one map as 1"""
        self._offer = ([(self.KEY, key)] if first else []) + [(self.VALUE % (i if first else 1), v) for i, v in enumerate(values)]


class AttentionDense(_Attention):
    """the attention tensor [b, n*hw, h, w] in one launch each of energy GEMM, softmax and - per map - weighted sums; attention_module
    hands out the TENSOR and wraps it again when it comes back (tensor=).  Two flavours, whose bits differ by the order of one fp32
    sum: the eager pass reduces the tensor for atn_vis / ref_idx, a session's kept frame (mass_from_softmax) takes both from the
    masses the softmax launch writes (ops.softmax_channels groups)."""

    def __init__(self, b, n, hw, h, w, query=None, kmat=None, tensor=None, mass_from_softmax=False):
        _Attention.__init__(self, b, n, hw, h, w)
        self.query, self.kmat, self.tensor, self.mass_from_softmax = query, kmat, tensor, mass_from_softmax

    def handle(self):
        return self.tensor

    def attend(self, values, want_mass=True):
        if want_mass:
            energy_t = ops.batch_conv(self.query, self.kmat, allow_half=False)                   # [b, n*hw, h, w]
            if self.mass_from_softmax:
                self.tensor, self.mass = ops.softmax_channels(energy_t, groups=self.n)
            else:
                self.tensor = ops.softmax_channels(energy_t)
        xmats = [_xmat(v, self.b, self.n, self.hw) for v in values]
        self._offers(want_mass, self.kmat, xmats)
        return [ops.batch_conv(self.tensor, xm, allow_half=False) for xm in xmats]              # [b, c, h, w]

    def atn_vis(self):
        if self.mass is not None:
            return _Attention.atn_vis(self)
        return self.tensor.reshape(self.b, self.n, self.hw, self.h, self.w).sum(2)[-1:, 0:1]

    def ref_idx(self):
        if self.mass is not None:
            return _Attention.ref_idx(self)
        return torch.argmax(self.tensor.reshape(self.b, self.n, -1).sum(2), dim=1)


def _attention_state(atn, n):
    """the state behind what attention_module handed out as `atn` (the dense kind hands out its attention tensor)"""
    if not torch.is_tensor(atn):
        return atn
    b, nhw, h, w = atn.shape
    return AttentionDense(b, n, nhw // n, h, w, tensor=atn)


class AttentionBands(_Attention):
    """the attention in query bands (attention_band_plan): the dense kind's three launches per band, on the same values, against
    kmat / xmat operands prepared once.  Without autograd ONE band of energy lives at a time - the softmax runs in place - in a
    buffer reused across the bands (band_buffer(numel, device): a session's static one), the masses come out of the softmax launch
    and a later call runs the bands again.  With autograd every band is the differentiable chain of the dense kind on a slice of
    the query: its attention is saved for backward, so the bands stay alive (`bands`) and a later call re-uses them."""

    def __init__(self, plan, b, n, hw, h, w, query=None, kmat=None, band_buffer=None):
        _Attention.__init__(self, b, n, hw, h, w)
        self.plan, self.query, self.kmat, self.band_buffer = plan, query, kmat, band_buffer
        self.bands = None            # [attention of band i] (autograd mode)

    def attend(self, values, want_mass=True):
        xmats = [_xmat(v, self.b, self.n, self.hw) for v in values]
        self._offers(want_mass, self.kmat, xmats)
        if self.bands is not None or (want_mass and torch.is_grad_enabled()):
            return self._attend_grad(xmats)
        if torch.is_grad_enabled():
            raise RuntimeError("banded attention: the attention of this pass was not kept for a second feature map")
        return self._attend_nograd(xmats)

    def _attend_nograd(self, xmats):
        b, n, hw, h, w = self.b, self.n, self.hw, self.h, self.w
        query = to_nhwc(self.query.detach())
        kop = ops.batch_conv_operand(self.kmat)
        xops = [ops.batch_conv_operand(xm) for xm in xmats]
        outs = [empty_nhwc(b, xm.shape[1], h, w, query) for xm in xmats]
        mass = torch.empty((b, h, w, n), dtype=torch.float32, device=query.device)
        need = max((s1 - s0) * (r1 - r0) for s0, s1, r0, r1 in self.plan) * w * n * hw
        buf = (self.band_buffer(need, query.device) if self.band_buffer is not None
               else torch.empty(need, dtype=torch.float32, device=query.device))
        for s0, s1, r0, r1 in self.plan:
            s, rows = s1 - s0, r1 - r0
            e = buf[:s * rows * w * n * hw].view(s, rows, w, n * hw).permute(0, 3, 1, 2)
            ops.batch_conv_band(query[s0:s1, :, r0:r1], kop, s0, out=e)
            ops.softmax_channels(e, groups=n, out=e, mass=mass[s0:s1, r0:r1])
            for o, xop in zip(outs, xops):
                ops.batch_conv_band(e, xop, s0, out=o[s0:s1, :, r0:r1])
        self.mass = mass
        return outs

    def _attend_grad(self, xmats):
        """the masses are detached reductions of each band; the outputs are assembled by ONE concatenation of [pixels, c] pieces - the
        bands are consecutive pieces of channels-last memory"""
        b, n, hw, h, w = self.b, self.n, self.hw, self.h, self.w
        first = self.bands is None
        bands, pieces, masses = [] if first else self.bands, [[] for _ in xmats], []
        for i, (s0, s1, r0, r1) in enumerate(self.plan):
            s, rows = s1 - s0, r1 - r0
            if first:
                bands.append(ops.softmax_channels(ops.batch_conv(self.query[s0:s1, :, r0:r1], self.kmat[s0:s1], allow_half=False)))
                masses.append(bands[i].detach().reshape(s, n, hw, rows * w).sum(2).permute(0, 2, 1).reshape(s * rows * w, n))
            for p, xm in zip(pieces, xmats):
                o = ops.batch_conv(bands[i], xm[s0:s1], allow_half=False)
                p.append(o.permute(0, 2, 3, 1).reshape(s * rows * w, o.shape[1]))
        if first:
            self.bands, self.mass = bands, torch.cat(masses, 0).view(b, h, w, n)
        return [torch.cat(p, 0).view(b, h, w, -1).permute(0, 3, 1, 2) for p in pieces]


class AttentionFused(_Attention):
    """the streaming attention (ops.attention_fused; grad: its differentiable form ops.attention_fused_grad) on the encoders' outputs as
    they lie in memory: ONE launch for the one or two maps of a call, no kmat / xmat arrangement, no band plan, no energy or attention
    tensor.  A later call walks the same query / key again; in the differentiable pass autograd adds the two contributions to them."""
    KEY, VALUE = 'key', 'val%d'

    def __init__(self, b, n, hw, h, w, query=None, key=None, grad=False):
        _Attention.__init__(self, b, n, hw, h, w)
        self.query, self.key, self.grad = query, key, grad

    def attend(self, values, want_mass=True):
        op = ops.attention_fused
        if self.grad and torch.is_grad_enabled():
            if not want_mass and not ops.attention_fused_grad_supported(self.query, self.key, values, self.n):
                raise RuntimeError("fused attention: the backward kernels do not serve a second feature map of %d channels: "
                                   "announce it before the first call" % values[0].shape[1])
            op = ops.attention_fused_grad
        elif not want_mass and torch.is_grad_enabled():
            raise RuntimeError("fused attention: the attention of this pass was not kept for a second feature map")
        outs, mass = op(self.query, self.key, values, self.n, want_mass=want_mass)
        if want_mass:
            self.mass = mass
        self._offers(want_mass, self.key, values)
        return outs


class AttentionFusedHalf(_Attention):
    """the streaming attention on the f16 matrix cores (ops.attention_fused_half; inference only): the reference side is prepared
    once - by this pass (`key`: ops.attention_half_prepare, one launch) or by a session's frame 0 (`prepared`: what it kept) - and
    every call is ONE launch for its one or two maps.  A later call for a map the first was not told of prepares and walks again."""
    KEY, VALUE = 'half', 'half_val%d'

    def __init__(self, b, n, hw, h, w, query=None, key=None, prepared=None):
        _Attention.__init__(self, b, n, hw, h, w)
        self.query, self.key, self.prepared = query, key, prepared

    def attend(self, values, want_mass=True):
        if torch.is_grad_enabled():
            raise RuntimeError("half fused attention is an inference path: autograd is on")
        prepared = self.prepared if want_mass else None
        if prepared is None:
            prepared = ops.attention_half_prepare(self.key, values, self.n)
        outs, mass = ops.attention_fused_half(self.query, prepared, want_mass=want_mass)
        if want_mass:
            self.mass = mass
        self._offers(want_mass, prepared, prepared.vts)          # (the operand object: the planes and the first call's maps)
        return outs


class FewShotGenerator(nn.Module):
    """Reference generator.py:20-454 without the KLD branch; n_shot >= 1 (with more than one reference image the attention module
    of generator.py:291-316 merges the reference features).  use_label_ref 'mul' (two encoders, softmax-pooled channel products
    feed the weight generators) or 'concat' (one encoder on [image | label], every weight generator reads a 32 x 32 adaptive
    average pool of a feature map: ops.pool_rows); adaptive_conv (generated conv_0 / conv_1 / conv_s of the adaptive decoder
    blocks) needs 'concat', as it does in the reference."""
    POOL = 32            # generator.py:54 sh_fix = sw_fix

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        if getattr(opt, 'lambda_kld', 0) > 0:
            # the reference computes mu / logvar but its loss collector never reads them, and the forward pass draws randn noise
            raise NotImplementedError("lambda_kld > 0: the KLD branch is outside the hot-path scope")
        self.n_shot = getattr(opt, 'n_shot', 1)
        self.n_downsample_A = getattr(opt, 'n_downsample_A', 2)
        use_label_ref = getattr(opt, 'use_label_ref', 'mul')
        if use_label_ref not in ('mul', 'concat'):
            raise NotImplementedError("use_label_ref = %r: only 'mul' and 'concat'" % (use_label_ref,))
        if getattr(opt, 'res_for_ref', False):
            raise NotImplementedError("res_for_ref: only SPADEConv2d reference encoders are on the hot path")
        self.concat_label_ref = use_label_ref == 'concat'
        self.adap_conv = bool(getattr(opt, 'adaptive_conv', False))
        if self.adap_conv and not self.concat_label_ref:
            # the reference builds the fc_conv_* MLPs for ch_out inputs but feeds them encoded_ref[i] with ch_in channels
            # (generator.py:104,412) and fails in the first Linear
            raise ValueError("--adaptive_conv needs --use_label_ref concat, as in the reference (its weight generators fail on "
                             "the 'mul' encoding)")
        exact = str(getattr(opt, 'amp', '') or '').lower() in ('', 'o0', 'fp32', 'f32')
        if (self.concat_label_ref or self.adap_conv) and not exact:
            raise NotImplementedError("use_label_ref = 'concat' / adaptive_conv under --amp (exact fp32 only)")
        # --norm_G / --norm_F (generator.py:32,62,469): batch or instance statistics in the decoder's SPADE layers and, with 'spade'
        # dropped (norm_ref), in every SPADEConv2d encoder; the flow network's layers follow norm_F
        self.norm = norm = getattr(opt, 'norm_G', NORMS_G[0])
        norm_F = getattr(opt, 'norm_F', NORMS_F[0])
        norm_kind(norm, spade=True)
        norm_kind(norm_F)
        norm_ref = norm.replace('spade', '')
        if not exact and (norm != NORMS_G[0] or norm_F != NORMS_F[0]):
            raise NotImplementedError("norm_G = %r / norm_F = %r under --amp (the half-precision SPADE forms reduce batch statistics "
                                      "only)" % (norm, norm_F))
        if opt.conv_ks != 3:
            raise NotImplementedError("conv_ks = %r: only 3 (the reference hard-codes padding 1 and a 3x3 get_conv_weights)"
                                      % (opt.conv_ks,))
        if opt.spade_ks not in (1, 3):
            raise NotImplementedError("spade_ks = %r: only 1 and 3" % (opt.spade_ks,))
        if opt.embed_ks not in (1, 3):
            raise NotImplementedError("embed_ks = %r: only 1 and 3" % (opt.embed_ks,))
        if opt.spade_ks != 1 and str(getattr(opt, 'amp', '') or '').lower() not in ('', 'o0', 'fp32', 'f32'):
            raise NotImplementedError("spade_ks = 3 under --amp (the 3x3 SPADE kernel is exact fp32 only)")
        self.spade_ks, self.embed_ks = opt.spade_ks, opt.embed_ks
        self.n_downsample_G = n = opt.n_downsample_G
        nf = opt.ngf
        nf_max = min(1024, nf * (2 ** n))
        self.ch = ch = [min(nf_max, nf * (2 ** i)) for i in range(n + 2)]
        self.spade_combine = opt.spade_combine
        self.n_sc_layers = opt.n_sc_layers
        self.add_raw_output_loss = getattr(opt, 'add_raw_output_loss', False) and opt.spade_combine
        ch_hidden = []
        for i in range(n + 1):
            ch_hidden += [[ch[i]]] if not self.spade_combine or i >= self.n_sc_layers else [[ch[i]] * 3]
        self.ch_hidden = ch_hidden
        self.adap_spade = opt.adaptive_spade
        self.adap_embed = opt.adaptive_spade and not getattr(opt, 'no_adaptive_embed', False)
        self.n_adaptive_layers = opt.n_adaptive_layers if opt.n_adaptive_layers != -1 else n
        self.n_fc_layers = opt.n_fc_layers
        input_nc = opt.label_nc if opt.label_nc != 0 else opt.input_nc
        concat = self.concat_label_ref
        self.ref_img_first = SPADEConv2d(opt.output_nc + (input_nc if concat else 0), nf, norm=norm_ref)
        if not concat:
            self.ref_label_first = SPADEConv2d(input_nc, nf, norm=norm_ref)
        for i in range(n):
            setattr(self, 'ref_img_down_%d' % i, SPADEConv2d(ch[i], ch[i + 1], stride=2, norm=norm_ref))
            setattr(self, 'ref_img_up_%d' % i, SPADEConv2d(ch[i + 1], ch[i], norm=norm_ref))
            if not concat:
                setattr(self, 'ref_label_down_%d' % i, SPADEConv2d(ch[i], ch[i + 1], stride=2, norm=norm_ref))
                setattr(self, 'ref_label_up_%d' % i, SPADEConv2d(ch[i + 1], ch[i], norm=norm_ref))
        if self.adap_spade or self.adap_conv:
            for i in range(self.n_adaptive_layers):
                ch_in, ch_out = ch[i], ch[i + 1]
                ch_h = ch_hidden[i][0]
                names, outs = [], []
                if self.adap_spade:
                    names += ['fc_spade_0', 'fc_spade_1', 'fc_spade_s']
                    sk2, ek2 = self.spade_ks ** 2, self.embed_ks ** 2          # generator.py:83-95
                    outs += [(ch_h * sk2 + 1) * 2, (ch_h * sk2 + 1) * (1 if ch_in != ch_out else 2), (ch_h * sk2 + 1) * 2]
                    if self.adap_embed:
                        names.append('fc_spade_e')
                        outs.append(ch_in * ek2 + 1)
                if self.adap_conv:                                            # generator.py:96-101
                    names += ['fc_conv_0', 'fc_conv_1', 'fc_conv_s']
                    outs += [ch_out * 9 + 1, ch_in * 9 + 1, ch_out + 1]
                # generator.py:104: under 'concat' every MLP reads one pooled POOL x POOL map per row
                fc_in = ch_out if not concat else self.POOL * self.POOL
                for name, fo in zip(names, outs):
                    layers = [Linear(fc_in, ch_out), _Slot()]
                    for _ in range(1, self.n_fc_layers):
                        layers += [Linear(ch_out, ch_out), _Slot()]
                    layers += [Linear(ch_out, fo)]
                    setattr(self, '%s_%d' % (name, i), _seq(*layers))
        self.label_embedding = LabelEmbedder(opt, input_nc, opt.netS,
                                             params_free_layers=(self.n_adaptive_layers if self.adap_embed else 0))
        for i in reversed(range(n + 1)):
            setattr(self, 'up_%d' % i, SPADEResnetBlock(ch[i + 1], ch[i], hidden_nc=ch_hidden[i], spade=True,
                                                       norm_params_free=(self.adap_spade and i < self.n_adaptive_layers),
                                                       spade_ks=self.spade_ks,
                                                       conv_params_free=(self.adap_conv and i < self.n_adaptive_layers), norm=norm))
        self.conv_img = Conv2d(nf, 3, 3, padding=1)
        if self.n_shot > 1:                # generator.py:128-134: key / query encoders of the attention module
            self.atn_query_first = SPADEConv2d(input_nc, nf, norm=norm_ref)
            self.atn_key_first = SPADEConv2d(input_nc, nf, norm=norm_ref)
            for i in range(self.n_downsample_A):
                setattr(self, 'atn_key_%d' % i, SPADEConv2d(ch[i], ch[i + 1], stride=2, norm=norm_ref))
                setattr(self, 'atn_query_%d' % i, SPADEConv2d(ch[i], ch[i + 1], stride=2, norm=norm_ref))
        self._sn_group, self._sn_count = None, -1
        self.warp_prev = False
        self.warp_ref = opt.warp_ref and not getattr(opt, 'for_face', False)
        if self.warp_ref:
            self.flow_network_ref = FlowGenerator(opt, 2)
            if self.spade_combine:
                self.img_ref_embedding = LabelEmbedder(opt, opt.output_nc + 1, opt.sc_arch)

    # -- temporal extension (reference generator.py:153-179) -------------------------------------------------------
    def init_temporal_network(self):
        opt = self.opt
        self.warp_prev = True
        self.sep_prev_flownet = opt.sep_flow_prev or (opt.n_frames_G != 2) or not opt.warp_ref
        self.sep_prev_embedding = self.spade_combine and (not opt.no_sep_warp_embed or not opt.warp_ref)
        dev = self.conv_img.weight.device
        if self.sep_prev_flownet:
            self.flow_network_temp = FlowGenerator(opt, opt.n_frames_G).to(dev)
        else:
            self.flow_network_temp = self.flow_network_ref
        if self.spade_combine:
            if self.sep_prev_embedding:
                self.img_prev_embedding = LabelEmbedder(opt, opt.output_nc + 1, opt.sc_arch).to(dev)
            else:
                self.img_prev_embedding = self.img_ref_embedding
        if self.warp_ref:
            if self.sep_prev_flownet:
                self.load_pretrained_net(self.flow_network_ref, self.flow_network_temp)
            if self.sep_prev_embedding:
                self.load_pretrained_net(self.img_ref_embedding, self.img_prev_embedding)
            self.flow_temp_is_initalized = True

    @staticmethod
    def load_pretrained_net(net_src, net_dst):
        src, dst = net_src.state_dict(), net_dst.state_dict()
        for k, v in src.items():
            if k in dst and dst[k].size() == v.size():
                dst[k] = v
        net_dst.load_state_dict(dst)

    # -- weight generation ---------------------------------------------------------------------------------------------
    def _mlp(self, name, i, rows):
        layers = getattr(self, '%s_%d' % (name, i))
        x = rows
        last = len(layers) - 1
        for k in range(0, last, 2):
            x = layers[k](x, act=ACT_LRELU)
        return layers[last](x)

    @staticmethod
    def _pairs(f, npairs, cout, cin, k=1):
        """f [b, L] -> npairs x [weight [b, cout, cin, k, k], bias [b, cout]] read off the front of each row
        (generator.py reshape_weight slices the flattened FC output the same way).  One split instead of nested slicing:
        its backward is ONE concatenation (ops.split_cols) instead of a zero-fill + copy + add per slice."""
        sizes = [cout * cin * k * k, cout] * npairs
        rest = f.shape[1] - sum(sizes)
        parts = ops.split_cols(f, sizes + ([rest] if rest > 0 else []))
        b = f.shape[0]
        return [[parts[2 * j].reshape(b, cout, cin, k, k), parts[2 * j + 1]] for j in range(npairs)]

    _MLP_NAMES = ('fc_spade_e', 'fc_spade_0', 'fc_spade_1', 'fc_spade_s')
    _CONV_MLP_NAMES = ('fc_conv_0', 'fc_conv_1', 'fc_conv_s')

    def _mlp_names(self):
        return self._MLP_NAMES if self.adap_embed else self._MLP_NAMES[1:]

    def _mlp_bank(self, feats, conv_feats=()):
        """All weight-generator MLPs of all adaptive levels, advanced layer by layer with one grouped launch per layer
        (ops.mlp_bank) instead of one small launch per Linear; {(name, level): FC output} or None when the grouped path does
        not apply (no optimiser-owned layouts yet, narrow-operand modes, FSV_CONV_GROUPS=0).  feats[i] feeds the fc_spade_* chains
        of level i, conv_feats[i] the fc_conv_* chains; a tensor that feeds several levels enters the bank once (its gradient is
        then summed inside it, in chain order)."""
        rows, slot = [], {}

        def rows_of(f):
            if id(f) not in slot:
                slot[id(f)] = len(rows)
                rows.append(f.reshape(f.shape[0] * f.shape[1], -1))
            return slot[id(f)]
        chains, keys = [], []
        for i in range(max(len(feats), len(conv_feats))):
            for names, fs in ((self._mlp_names(), feats), (self._CONV_MLP_NAMES, conv_feats)):
                if i >= len(fs):
                    continue
                r = rows_of(fs[i])
                for name in names:
                    layers = getattr(self, '%s_%d' % (name, i))
                    chains.append((r, [layers[k] for k in range(0, len(layers), 2)]))
                    keys.append((name, i))
        outs = ops.mlp_bank(rows, chains)
        return None if outs is None else dict(zip(keys, outs))

    def get_SPADE_weights(self, feat, i, fc=None):
        """fc: {(name, level): FC output rows} from _mlp_bank, or None: run this level's MLPs here"""
        ch_in, ch_out = self.ch[i], self.ch[i + 1]
        ch_h = self.ch_hidden[i][0]
        b = feat.shape[0]
        rows = feat.reshape(b * feat.shape[1], -1) if fc is None else None

        def mlp(name):
            return fc[(name, i)] if fc is not None else self._mlp(name, i, rows)
        embedding_weights = None
        if self.adap_embed:
            fe = mlp('fc_spade_e').view(b, -1)
            # the reference drops the trailing ch_in entries, then reads weight | bias off what is left: the same split
            embedding_weights = self._pairs(fe, 1, ch_in, ch_out, self.embed_ks)[0]

        def two(name, co):
            f = mlp(name).view(b, -1)
            return self._pairs(f, 2, co, ch_h, self.spade_ks)
        return embedding_weights, [two('fc_spade_0', ch_out), two('fc_spade_1', ch_in), two('fc_spade_s', ch_out)]

    def get_conv_weights(self, feat, i, fc=None):
        """generator.py:276-289: [weight, bias] of conv_0 [ch_in <- ch_out, 3x3], conv_1 [ch_in <- ch_in, 3x3] and conv_s
        [ch_in <- ch_out, 1x1] of block up_i.  reshape_weight reads the weight off the front of the flattened FC output and ch_in
        biases off its end; the output is exactly that long, so the split of _pairs is the same"""
        ch_in, ch_out = self.ch[i], self.ch[i + 1]
        b = feat.shape[0]
        rows = feat.reshape(b * feat.shape[1], -1) if fc is None else None

        def one(name, ci, k):
            f = (fc[(name, i)] if fc is not None else self._mlp(name, i, rows)).view(b, -1)
            return self._pairs(f, 1, ch_in, ci, k)[0]
        return [one('fc_conv_0', ch_out, 3), one('fc_conv_1', ch_in, 3), one('fc_conv_s', ch_out, 1)]

    def attention_encode(self, img, name):
        x = getattr(self, name + '_first')(img)
        for i in range(self.n_downsample_A):
            x = getattr(self, '%s_%d' % (name, i))(x)
        return x

    def attention_module(self, x, label, label_ref, attention=None):
        """generator.py:298-316.  energy = key^T query over all N*HW reference positions, softmax over them, then the
        attention-weighted sum of the N reference feature maps.  Both batched matrix products run on the gather-GEMM
        kernel as per-sample 1x1 convolutions over the h x w query positions, kept in the transposed arrangement
        attention_t[b, (n, p_key), y, x] so that the softmax is the channel softmax kernel.
        The first call of a pass (attention None) chooses the kind that runs - the half streaming kind in an inference pass where
        attention_half_switch says so, streaming where its switch is set and the kernels serve
        the shape, query bands where attention_band_plan asks for them, else dense - and attends x together with a second feature map
        reference_encoding announced (self._atn_second: the label features under use_label_ref 'mul'; the dense kind leaves it to
        its own call).  The later call attention_module(xl, None, None, atn) picks that result up, or attends xl by what was kept."""
        n = self.n_shot
        b, (c, h, w) = x.shape[0] // n, x.shape[1:]
        hw = h * w
        if attention is not None:
            atn = _attention_state(attention, n)
            if atn.second is not None and atn.second[0] is x:
                return atn.second[1], attention, atn.atn_vis()
            outs = atn.attend([x], want_mass=False)
        else:
            second = self.__dict__.get('_atn_second', None)
            cvs = [c] + ([second.shape[1]] if second is not None else [])
            half = attention_half_switch(self) and ops.attention_fused_half_serves(b, n, hw, c, cvs)
            fused = not half and attention_fused_switch(self) and ops.attention_fused_serves(b, n, hw, c, cvs)
            grad = not (half or fused) and attention_fused_grad_switch() and ops.attention_fused_grad_serves(b, n, hw, c, cvs)
            plan = None if half or fused or grad else attention_band_plan(b, n, hw, h, w)
            key = self.attention_encode(label_ref, 'atn_key')            # [b*n, c, h, w]
            query = self.attention_encode(label, 'atn_query')            # [b, c, h, w]
            if half:
                atn = AttentionFusedHalf(b, n, hw, h, w, query, key)
            elif fused or grad:
                atn = AttentionFused(b, n, hw, h, w, query, key, grad)
            elif plan is not None:
                atn = AttentionBands(plan, b, n, hw, h, w, query, _kmat(key, b, n, hw))
            else:
                atn, second = AttentionDense(b, n, hw, h, w, query, _kmat(key, b, n, hw)), None
            if second is not None:
                self.__dict__.pop('_atn_second')
            outs = atn.attend([x] + ([second] if second is not None else []))
            if second is not None:
                atn.second = (second, outs[1])
        # an infer.InferenceSession with keep_references collects the operands of the reference side while frame 0 runs (the tensors
        # this pass builds anyway: nothing more is launched here)
        sink = getattr(self, '_kept_refs', None) if not torch.is_grad_enabled() else None
        if sink is not None:
            for name, t in atn.operands():
                sink.collect(name, t)
        return outs[0], atn.handle(), atn.atn_vis()

    def attention_module_kept(self, kept, label):
        """attention_module on the operands an infer.InferenceSession kept from frame 0 (`keep_references`): after a half streaming
        frame 0 kept.half, the prepared half operands; after a streaming frame 0
        kept.key / kept.vals, the key and reference features in their own NHWC memory; otherwise kept.kmat, the key encoding of the
        reference labels, and kept.xmats, the reference features that enter the attention (image encoder, then label encoder), each in
        the arrangement its GEMM reads - in query bands where the plan asks for them, the band buffer the session's own (static under a
        captured graph).  Per frame: the query encoder and the kind's launches, the same launches on the same values as
        attention_module, so the same bits; the masses come out of the softmax launch, the attention tensor is not read again.
        Returns ([attended image feature, attended label feature or None], atn_vis, ref_idx)."""
        query = self.attention_encode(label, 'atn_query')
        n = self.n_shot
        b, (h, w) = query.shape[0], query.shape[2:]
        hw = h * w
        if kept.half is not None:        # (the prepared operands of ops.attention_fused_half: no prep launch in a steady frame)
            atn, values = AttentionFusedHalf(b, n, hw, h, w, query, prepared=kept.half), kept.half.vts
        elif kept.key is not None:
            atn, values = AttentionFused(b, n, hw, h, w, query, kept.key), kept.vals
        else:
            plan, values = attention_band_plan(b, n, hw, h, w), kept.xmats
            if plan is not None:
                atn = AttentionBands(plan, b, n, hw, h, w, query, kept.kmat, kept.band_buffer)
            else:
                atn = AttentionDense(b, n, hw, h, w, query, kept.kmat, mass_from_softmax=True)
        outs = atn.attend(values)
        return outs + [None] * (2 - len(outs)), atn.atn_vis(), atn.ref_idx()

    def reference_encoding(self, img_ref, label_ref, encode=True, label=None):
        n = self.n_downsample_G
        # (the two encoders as parallel branches of the captured graph: +2 ... 3 ms in round 2, re-measured in round 6 on the final
        # kernels: 42.32 / 42.65 -> 43.50 / 43.51 ms per step - profiles/r06_step_ab_schedule.txt; not kept)
        concat = self.concat_label_ref
        # the reference side a session kept at frame 0 (infer.InferenceSession keep_references): in eval() every layer of the
        # encoders is per sample, so levels 0 .. A - 1 and the key encoder give the same tensors on every frame of the sequence
        kept = getattr(self, '_kept_refs', None)
        if kept is not None and not (kept.ready and self.n_shot > 1 and not torch.is_grad_enabled() and not self.training):
            kept = None
        first = 0
        atn = atn_vis = ref_idx = None
        if kept is not None:
            (x, xl), atn_vis, ref_idx = self.attention_module_kept(kept, label)
            first = self.n_downsample_A
        elif concat:             # generator.py:342-345: one encoder on [image | label]
            x = self.ref_img_first(ops.cat_channels([img_ref, label_ref]))
            xl = None
        else:
            x = self.ref_img_first(img_ref)
            xl = self.ref_label_first(label_ref)
        for i in range(first, n):
            x = getattr(self, 'ref_img_down_%d' % i)(x)
            if not concat:
                xl = getattr(self, 'ref_label_down_%d' % i)(xl)
            if kept is None and self.n_shot > 1 and i == self.n_downsample_A - 1:          # generator.py:359-366
                if not concat:           # (banded attention: the label features are attended in the image features' band loop)
                    self._atn_second = xl
                try:
                    x, atn, atn_vis = self.attention_module(x, label, label_ref)
                finally:
                    self.__dict__.pop('_atn_second', None)
                if not concat:
                    xl, _, _ = self.attention_module(xl, None, None, atn)
                ref_idx = _attention_state(atn, self.n_shot).ref_idx()
        self._atn = (atn_vis, ref_idx)
        if not encode:           # generator.py:370: test-time frames after the first re-use the cached weights
            return x, None
        fi, fl = [x], [xl]
        for i in reversed(range(n)):
            fi.append(getattr(self, 'ref_img_up_%d' % i)(fi[-1]))
            if not concat:
                fl.append(getattr(self, 'ref_label_up_%d' % i)(fl[-1]))
        if concat:
            return x, self._pooled_rows(fi[::-1])
        return x, self._pooled(fi, fl)

    def _pooled_rows(self, feats):
        """'concat': what the weight generators read is nn.AdaptiveAvgPool2d((32, 32)) of the encoder's feature maps themselves,
        one row per channel (generator.py:248,278, reshape_embed_input).  One pooled tensor [b, c, 1024] per feature map and pass,
        shared by the fc_spade_* chains of level l - 1 and the fc_conv_* chains of level l (the reference pools the map once for
        each; the values are the same); maps no generator reads are not pooled."""
        n, nl = self.n_downsample_G, self.n_adaptive_layers
        used = set(min(n, i + 1) for i in range(nl) if self.adap_spade) | set(min(n, i) for i in range(nl) if self.adap_conv)
        return [ops.pool_rows(f, self.POOL, self.POOL).view(f.shape[0], f.shape[1], self.POOL * self.POOL) if l in used else None
                for l, f in enumerate(feats)]

    @staticmethod
    def _pooled(fi, fl):
        enc = []
        for a, l in zip(fi, fl):
            b, c, h, w = a.shape
            sm = ops.softmax_channels(l)
            # prod[b, i, j] = sum_p a[b, i, p] * sm[b, j, p]  as a per-sample 1x1 "convolution" on the gather-GEMM
            # kernel: pixels = image channels i, input channels = positions p, generated weights = softmax rows j
            a_rows = a.reshape(b, c, 1, h * w).permute(0, 3, 1, 2)              # logical [b, hw, c, 1]
            wts = sm.reshape(b, c, h * w, 1, 1)
            prod = ops.batch_conv(a_rows, wts, allow_half=False)                                    # logical [b, c(j), c(i), 1]
            enc.append(prod.permute(0, 2, 1, 3))                                  # [b, c(i), c(j), 1]
        return enc[::-1]

    def weight_generation(self, img_ref, label_ref, label, t=0, label_maps_elsewhere=False):
        """returns (x, label maps, SPADE weights, conv weights); with `label_maps_elsewhere` the second entry is the generated
        embedding weights instead (label_embedding.encode_maps runs next to the flow network, forward() finishes with decode_maps)"""
        b, n, c, h, w = img_ref.shape
        img_ref, label_ref = img_ref.reshape(b * n, -1, h, w), label_ref.reshape(b * n, -1, h, w)
        # generator.py:370,403-416: at test time (isTrain False, one reference) the generated weights of frame 0 are kept
        # and every later frame only runs the down path of the reference encoder
        fresh = bool(self.opt.isTrain) or n > 1 or t == 0
        kept_x = getattr(self, '_frozen_x', None) if not fresh else None
        if kept_x is not None:
            # an infer.InferenceSession keeps frame 0's deepest reference feature with the generated weights: with one reference
            # and frozen weights the encoder's down path gives the same tensor on every frame
            x, enc, self._atn = kept_x, None, (None, None)
        else:
            x, enc = self.reference_encoding(img_ref, label_ref, encode=fresh, label=label)
        cut2 = getattr(self, 'bwd_cut2', None)
        if cut2 is not None and fresh and torch.is_grad_enabled():
            # second stage boundary (three-piece backward): what the reference encoders hand on - the deepest feature map and
            # the pooled products ('concat': the pooled rows, not the full-size maps) the weight generators read - becomes
            # detached leaves; the encoders' backward is the third piece
            cut2.begin_forward()
            x, enc = cut2.split((x, enc))
        if fresh:
            embed_w, norm_w, conv_w = [], [], []
            if self.adap_spade or self.adap_conv:
                nl = self.n_adaptive_layers
                feats = [enc[min(len(enc) - 1, i + 1)] for i in range(nl)] if self.adap_spade else []
                conv_feats = [enc[min(len(enc) - 1, i)] for i in range(nl)] if self.adap_conv else []         # generator.py:412
                fc = self._mlp_bank(feats, conv_feats)
                for i in range(nl):
                    if self.adap_spade:
                        e, nw = self.get_SPADE_weights(feats[i], i, fc)
                        embed_w.append(e)
                        norm_w.append(nw)
                    if self.adap_conv:
                        conv_w.append(self.get_conv_weights(conv_feats[i], i, fc))
            if not self.opt.isTrain:
                self._cached_weights = (embed_w, norm_w, conv_w)         # generator.py:415-416
                self._cached_x = x
        else:
            embed_w, norm_w, conv_w = self._cached_weights
        embed_w = embed_w if self.adap_embed else None
        if label_maps_elsewhere:
            return x, embed_w, norm_w, conv_w
        return x, self.label_embedding(label, weights=embed_w), norm_w, conv_w

    def forward_face(self, label, label_refs, img_refs, img_coarse):
        """generator.py:232-242 (the --refine_face generator): the decoder starts from the encoding of the COARSE face
        (compute_kld with img_coarse, generator.py:321-325: reference-image encoder applied to it) instead of the
        reference image's; SPADE weights still come from the reference crops."""
        if self.adap_conv:
            # generator.py:232-238 hands the blocks no conv weights: their parameter-free convolutions return the input, and the
            # reference stops at the first block whose channel counts differ
            raise ValueError("--refine_face with --adaptive_conv: the reference's face generator passes no convolution weights")
        _, enc_label, norm_w, _ = self.weight_generation(img_refs, label_refs, label)
        # generator.py:321-325: under 'concat' the encoder reads [coarse face | label]
        x = self.ref_img_first(ops.cat_channels([img_coarse, label]) if self.concat_label_ref else img_coarse)
        for i in range(self.n_downsample_G):
            x = getattr(self, 'ref_img_down_%d' % i)(x)
        for i in range(self.n_downsample_G, -1, -1):
            nw = norm_w[i] if (self.adap_spade and i < self.n_adaptive_layers) else None
            x = getattr(self, 'up_%d' % i)(x, enc_label[i], nw, up=(i != self.n_downsample_G))
        return self.conv_img(ops.activation(x, ACT_LRELU), act=ACT_TANH)

    def flow_generation(self, label, label_ref, img_ref, prev):
        """generator.py:430-449.  The warp is fused with what consumes it (ops.warp_concat / ops.warp_blend, csrc/warp.hip):
        with --spade_combine the warped image and ds = cat([warp, mask]) come out of one launch here; otherwise the warp is
        left to the blend in forward() (`sources` carries the images to warp)."""
        label_prev, img_prev = prev
        flow, mask, warp, ds = [None, None], [None, None], [None, None], [None, None]
        sources = [None, None]
        if self.warp_ref:
            flow[0], mask[0] = self.flow_network_ref(label, label_ref, img_ref, for_ref=True)
            sources[0] = img_ref[:, :3]
        if self.warp_prev and label_prev is not None:
            flow[1], mask[1] = self.flow_network_temp(label, label_prev, img_prev)
            sources[1] = img_prev[:, -3:]
        if self.spade_combine:
            for k in range(2):
                if sources[k] is not None:
                    warp[k], ds[k] = ops.warp_concat(sources[k], flow[k], mask[k])
        self._warp_sources = sources
        return flow, mask, warp, ds

    def combine_embeddings(self, ds):
        """generator.py:218-225 (--spade_combine): SPADE maps from the warped reference / previous image"""
        if not self.spade_combine:
            return None
        return [self.img_ref_embedding(ds[0]), self.img_prev_embedding(ds[1]) if ds[1] is not None else None]

    def flow_branch(self, label, label_ref, img_ref, prev, with_label_maps=False):
        """everything of the forward pass that needs neither the reference encoders nor the generated weights: flow network,
        warp, the SPADE maps of the warped image and (with_label_maps) the weight-free part of the label embedding"""
        maps = None
        early = with_label_maps and _decode_early() and label.is_cuda
        if early:
            # round 6 (FSV_DECODE_EARLY=0: the old order): the label maps FIRST, with an event behind them - the other branch then
            # decodes them right behind its weight generators instead of behind the join of both branches.  In the replayed graph the
            # twelve small launches of decode_maps sat ~90 us apart behind that join in the generator-mode pass (a 0.7 ms hole in
            # profiles/r06_step_sequence.txt; back to back in the no-grad pass and, here, on the branch's own queue); unprofiled the
            # step gains 0.1 ms (profiles/r06_step_ab_schedule.txt) - most of that hole is the profiler's cross-queue cost
            maps = self.label_embedding.encode_maps(label)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(label.device))
            self._maps_ready = (ev, maps)
        flow, mask, warp, ds = self.flow_generation(label, label_ref, img_ref, prev)
        emb = self.combine_embeddings(ds)
        if with_label_maps and not early:
            maps = self.label_embedding.encode_maps(label)
        return flow, mask, warp, emb, maps

    def stage2_parameters(self):
        """parameters below the BackwardCut boundary of forward(): decoder blocks, output conv"""
        names = ('up_', 'conv_img')
        return [p for n, p in self.named_parameters() if n.startswith(names)]

    def stage3_parameters(self):
        """parameters above the SECOND boundary (three-piece backward, `bwd_cut2` on the outputs of reference_encoding): the
        reference encoders and the attention encoders - the last part of the network the backward pass reaches"""
        names = ('ref_img_', 'ref_label_', 'atn_')
        return [p for n, p in self.named_parameters() if n.startswith(names)]

    def _sn_update(self):
        if self._sn_group is None or self._sn_count != sum(1 for _ in self.modules()):
            self._sn_group = ops.SpectralGroup(spectral_layers(self))
            self._sn_count = sum(1 for _ in self.modules())
        self._sn_group.update(self.training)

    def forward(self, label, label_refs, img_refs, prev=(None, None), t=0, img_coarse=None):
        from .conv import stats_pass
        with stats_pass(label.device):          # a no-op inside Vid2VidModel.forward's pass; opens one for bare generator calls
            return self._forward(label, label_refs, img_refs, prev, t, img_coarse)

    def _forward(self, label, label_refs, img_refs, prev=(None, None), t=0, img_coarse=None):
        self._sn_update()
        if img_coarse is not None:
            return self.forward_face(label, label_refs, img_refs, img_coarse)
        if self.n_shot == 1 and label_refs.shape[1] == 1:
            # The flow branch (flow network, warp, the SPADE maps of the warped image) depends on nothing the reference
            # encoders / weight generators produce: two parallel branches (streams.fork).  With attention (n_shot > 1) it
            # needs ref_idx first.
            self._maps_ready = None

            def generate_and_decode():
                x, embed_w, norm_w, conv_w = self.weight_generation(img_refs, label_refs, label, t=t, label_maps_elsewhere=True)
                ready = self._maps_ready            # (set by the flow branch, which streams.fork issues first)
                if ready is None:
                    return x, embed_w, norm_w, conv_w, None
                ev, maps = ready
                cur = torch.cuda.current_stream(label.device)
                cur.wait_event(ev)
                streams._record(maps, cur)
                return x, embed_w, norm_w, conv_w, self.label_embedding.decode_maps(maps, embed_w)
            (x, embed_w, norm_w, conv_w, enc_label), (flow, mask, warp, emb, maps) = streams.fork(label, [
                generate_and_decode,
                lambda: self.flow_branch(label, label_refs[:, 0], img_refs[:, 0], prev, with_label_maps=True)])
            self._maps_ready = None
            if enc_label is None:
                enc_label = self.label_embedding.decode_maps(maps, embed_w)
            atn_vis, ref_idx = self._atn
        else:
            x, enc_label, norm_w, conv_w = self.weight_generation(img_refs, label_refs, label, t=t)
            atn_vis, ref_idx = self._atn
            label_ref, img_ref = pick_ref(label_refs, ref_idx), pick_ref(img_refs, ref_idx)
            flow, mask, warp, emb, _ = self.flow_branch(label, label_ref, img_ref, prev)
        cut = getattr(self, 'bwd_cut', None)
        if cut is not None and torch.is_grad_enabled():
            cut.begin_forward()
            # stage boundary (see BackwardCut): everything above is "stage 1", the decoder below is "stage 2"
            # (stage2_parameters)
            x, enc_label, norm_w, conv_w, flow, mask, warp, emb = cut.split((x, enc_label, norm_w, conv_w, flow, mask, warp, emb))
            enc_label = list(enc_label)
        # --add_raw_output_loss (generator.py:195, 202-205, 227): the last n_sc_layers blocks run a second time on the label
        # embedding alone (no warped-image maps) - same modules, so their spectral norms and BatchNorm running statistics take a
        # second update, as the reference's do
        enc_raw = [enc_label[i] for i in range(self.n_sc_layers)] if self.add_raw_output_loss else None
        x_raw = None
        if self.spade_combine:
            for i in range(self.n_sc_layers):
                enc_label[i] = [enc_label[i]] + [e[i] if e is not None else None for e in emb]
        for i in range(self.n_downsample_G, -1, -1):
            nw = norm_w[i] if (self.adap_spade and i < self.n_adaptive_layers) else None
            cw = conv_w[i] if (self.adap_conv and i < self.n_adaptive_layers) else None
            # generator.py:121-124: the nearest x2 up-sampling after block i + 1 is handed to block i (up=True), whose SPADE
            # kernels read through the up-sampling index
            if enc_raw is not None and i < self.n_sc_layers:
                if i == self.n_sc_layers - 1:
                    x_raw = x
                x_raw = getattr(self, 'up_%d' % i)(x_raw, enc_raw[i], nw, up=(i != self.n_downsample_G), feeds_norm=i > 0,
                                                   conv_weights=cw)
            x = getattr(self, 'up_%d' % i)(x, enc_label[i], nw, up=(i != self.n_downsample_G), feeds_norm=i > 0, conv_weights=cw)
        img_raw = self.conv_img(ops.activation(x, ACT_LRELU), act=ACT_TANH)
        if not self.spade_combine:
            img_final = img_raw
            sources = self._warp_sources
            warp = list(warp)
            if self.warp_ref:
                warp[0], img_final = ops.warp_blend(img_raw, sources[0], flow[0], mask[0])
            elif not self.warp_prev:
                img_raw = None
            if sources[1] is not None:
                warp[1], img_final = ops.warp_blend(img_final, sources[1], flow[1], mask[1])
        else:
            img_final = img_raw
            img_raw = self.conv_img(ops.activation(x_raw, ACT_LRELU), act=ACT_TANH) if x_raw is not None else None
        return img_final, flow, mask, img_raw, warp, None, None, atn_vis, ref_idx


class BackwardCut:
    """A stage boundary inside one forward pass, for backward passes that run in two pieces (graph_step / bench.py at
    N > 1: the gradients of the decoder stage are complete after the first piece and are all-reduced on a side stream
    while the second piece - the encoders, weight generators and the flow network - is still running).

    split() replaces every tensor that crosses the boundary by a detached leaf; `loss.backward()` then stops at the leaves
    (first piece), and backward_rest() continues from the recorded originals with the gradients the leaves collected."""

    # cuts that hold an unfinished second piece.  Every backward driver (model.loss_backward, graph_step, a caller's own
    # `.backward()` followed by finish_all()) completes them from here, so the forward pass that detached at the boundary -
    # not an attribute of whichever optimiser happens to be stepped - decides whether a second piece has to run.
    _live = weakref.WeakSet()

    def __init__(self):
        self.pairs = []

    def begin_forward(self):
        """a new forward pass supersedes the boundary tensors of one whose backward never ran"""
        self.pairs = []
        BackwardCut._live.discard(self)

    def split(self, obj):
        if torch.is_tensor(obj):
            if not obj.requires_grad:
                return obj
            leaf = obj.detach().requires_grad_(True)
            self.pairs.append((obj, leaf))
            BackwardCut._live.add(self)
            return leaf
        if isinstance(obj, (list, tuple)):
            return type(obj)(self.split(o) for o in obj)
        return obj

    def has_grads(self):
        """the first piece of THIS cut's backward pass has run and the second is still due"""
        return any(l.grad is not None for _, l in self.pairs)

    def backward_rest(self):
        """second piece: continue from the recorded originals with the gradients the leaves collected.  A cut whose leaves have
        no gradient yet stays registered: its own backward pass has not run (a G forward with grad followed by a D
        loss_backward - whose finish_all() reaches every live cut - and only then the G backward: round-3 advisor)."""
        outs = [o for o, l in self.pairs if l.grad is not None]
        grads = [l.grad for o, l in self.pairs if l.grad is not None]
        if not outs:
            return
        self.pairs = []
        BackwardCut._live.discard(self)
        torch.autograd.backward(outs, grads)

    def abandon(self):
        """drop the boundary tensors of a forward pass whose backward will never run (an interrupted graph capture)"""
        self.pairs = []
        BackwardCut._live.discard(self)

    @classmethod
    def finish_all(cls):
        """run the remaining pieces of every forward pass that detached at a stage boundary and whose first piece has run (a cut
        inside the region behind another cut gets its gradients from that one's piece: repeat until nothing moves)"""
        moved = True
        while moved:
            moved = False
            for cut in list(cls._live):
                if cut.has_grads():
                    cut.backward_rest()
                    moved = True

    @classmethod
    def abandon_all(cls):
        for cut in list(cls._live):
            cut.abandon()


# ------------------------------------------------------------------------------------------------ discriminator
class NLayerDiscriminator(nn.Module):
    """Reference discriminator.py:61-102 with norm 'spectralinstance': k4 p2 PatchGAN returning every feature."""

    def __init__(self, input_nc, ndf=64, n_layers=3, getIntermFeat=False, stride=2):
        super().__init__()
        self.getIntermFeat, self.n_layers = getIntermFeat, n_layers
        self.model0 = _seq(Conv2d(input_nc, ndf, 4, stride=stride, padding=2), _Slot())
        nf = ndf
        for n in range(1, n_layers):
            nf_prev, nf = nf, min(nf * 2, 512)
            setattr(self, 'model%d' % n, _seq(_seq(Conv2d(nf_prev, nf, 4, stride=stride, padding=2, bias=False, spectral=True),
                                                   InstanceNorm(nf)), _Slot()))
        nf_prev, nf = nf, min(nf * 2, 512)
        setattr(self, 'model%d' % n_layers, _seq(_seq(Conv2d(nf_prev, nf, 4, stride=1, padding=2, bias=False, spectral=True),
                                                      InstanceNorm(nf)), _Slot()))
        setattr(self, 'model%d' % (n_layers + 1), _seq(Conv2d(nf, 1, 4, stride=1, padding=2)))
        self._sn_group = None

    def forward(self, x, sn=None):
        """sn: None - one power iteration, then the pass (the reference's forward pre-hook); or the sigmas of an earlier
        begin_pass() - Vid2VidModel's G step runs the real and the generated images in separate passes that count as ONE
        forward of the reference's batched call."""
        snap = self.begin_pass() if sn is None else sn
        for l, c in snap:
            l._sig_cached = c
        try:
            return self._run(x)
        finally:
            for l, _ in snap:
                l._sig_cached = None

    def begin_pass(self):
        """one power iteration of every spectral layer; returns the (layer, sigma / u / v snapshot) list for forward(sn=...)"""
        if self._sn_group is None:
            self._sn_group = ops.SpectralGroup(spectral_layers(self))
        self._sn_group.update(self.training)
        snap = [(l, l._sig_cached) for l in self._sn_group.layers]
        for l, _ in snap:
            l._sig_cached = None
        return snap

    def _run(self, x):
        res = []
        x = self.model0[0](x, act=ACT_LRELU)
        res.append(x)
        for n in range(1, self.n_layers + 1):
            conv, norm = getattr(self, 'model%d' % n)[0]
            x = norm(conv(x, stats=-1), act=ACT_LRELU)
            res.append(x)
        x = getattr(self, 'model%d' % (self.n_layers + 1))[0](x)
        res.append(x)
        return res if self.getIntermFeat else res[-1]


class AdaptiveDiscriminator(NLayerDiscriminator):
    """Reference discriminator.py:104-209 (`--netD_subarch adaptive`): the first `adaptive_layers` convolutions take weights
    GENERATED from the reference image - encoder_n (k4 s2 p2 + LeakyReLU) on [ref label | ref image], adaptive average pooling of
    every encoded channel to (fineSize / 8 / aspect, fineSize / 8), one Linear per layer from the pooled map to a k4 x k4 filter
    row - applied per sample with stride 2, InstanceNorm (no affine) and LeakyReLU; the remaining layers are the spectral
    PatchGAN's.  Same attribute names / state_dict keys as the reference."""

    def __init__(self, opt, input_nc, ndf=64, n_layers=3, getIntermFeat=False, adaptive_layers=1):
        nn.Module.__init__(self)
        self.getIntermFeat, self.n_layers, self.adaptive_layers = getIntermFeat, n_layers, adaptive_layers
        self.input_nc, self.ndf = input_nc, ndf
        self.sw = opt.fineSize // 8
        self.sh = int(self.sw / opt.aspect_ratio)
        ch = self.sh * self.sw
        nf = ndf
        self.fc_0 = Linear(ch, input_nc * 16, spectral=False)
        self.encoder_0 = _seq(Conv2d(input_nc, ndf, 4, stride=2, padding=2), _Slot())
        for n in range(1, adaptive_layers):
            nf_prev, nf = nf, min(nf * 2, 512)
            setattr(self, 'fc_%d' % n, Linear(ch, nf_prev * 16, spectral=False))
            setattr(self, 'encoder_%d' % n, _seq(Conv2d(nf_prev, nf, 4, stride=2, padding=2), _Slot()))
        nf = ndf * (2 ** (adaptive_layers - 1))
        for n in range(adaptive_layers, n_layers + 1):
            nf_prev, nf = nf, min(nf * 2, 512)
            setattr(self, 'model%d' % n, _seq(_seq(Conv2d(nf_prev, nf, 4, stride=2 if n != n_layers else 1, padding=2, bias=False,
                                                          spectral=True), InstanceNorm(nf)), _Slot()))
        setattr(self, 'model%d' % (n_layers + 1), _seq(Conv2d(nf, 1, 4, stride=1, padding=2)))
        self._sn_group = None

    def forward(self, x, ref=None, sn=None):
        if ref is None:
            raise ValueError("the adaptive discriminator needs the reference [label | image] tensor")
        snap = self.begin_pass() if sn is None else sn
        for l, c in snap:
            l._sig_cached = c
        try:
            return self._run_adaptive(x, ref)
        finally:
            for l, _ in snap:
                l._sig_cached = None

    def _run_adaptive(self, x, ref):
        enc, r = [], ref
        for n in range(self.adaptive_layers):                       # encode (discriminator.py:186-190)
            r = getattr(self, 'encoder_%d' % n)[0](r, act=ACT_LRELU)
            enc.append(r)
        res = []
        nf, nf_prev = self.ndf, self.input_nc
        for n in range(self.adaptive_layers):                       # gen_conv_weights + batch_conv (discriminator.py:142-170,192-197)
            e = enc[n]
            b, ch = e.shape[0], e.shape[1]
            pooled = ops.adaptive_avgpool(e, self.sh, self.sw).reshape(b * ch, self.sh * self.sw)
            wgt = getattr(self, 'fc_%d' % n)(pooled).view(b, nf, nf_prev, 4, 4)
            x = ops.batch_conv(x, wgt, None, stride=2, allow_half=False)
            x = ops.norm_act(x, None, None, None, None, instance=True, eps=1e-5, act=ACT_LRELU)
            res.append(x)
            nf_prev, nf = nf, min(nf * 2, 512)
        for n in range(self.adaptive_layers, self.n_layers + 1):
            conv, norm = getattr(self, 'model%d' % n)[0]
            x = norm(conv(x, stats=-1), act=ACT_LRELU)
            res.append(x)
        x = getattr(self, 'model%d' % (self.n_layers + 1))[0](x)
        res.append(x)
        return res if self.getIntermFeat else res[-1]


class MultiscaleDiscriminator(nn.Module):
    """Reference discriminator.py:16-58 (subarch 'n_layers' or 'adaptive')."""

    def __init__(self, opt, input_nc, ndf=64, n_layers=3, num_D=1, getIntermFeat=False, stride=2, subarch='n_layers'):
        super().__init__()
        self.num_D, self.getIntermFeat, self.subarch = num_D, getIntermFeat, subarch
        for i in range(num_D):
            if subarch == 'adaptive':
                d = AdaptiveDiscriminator(opt, input_nc, ndf, n_layers, getIntermFeat, getattr(opt, 'adaptive_D_layers', 1))
            else:
                d = NLayerDiscriminator(input_nc, ndf, n_layers, getIntermFeat, stride)
            setattr(self, 'discriminator_%d' % i, d)

    def begin_pass(self):
        return [getattr(self, 'discriminator_%d' % i).begin_pass() for i in range(self.num_D)]

    def forward(self, x, ref=None, sn=None):
        result = []
        adaptive = self.subarch == 'adaptive'
        for i in range(self.num_D):
            d = getattr(self, 'discriminator_%d' % i)
            out = d(x, ref, sn=sn[i] if sn is not None else None) if adaptive else d(x, sn=sn[i] if sn is not None else None)
            result.append(out if self.getIntermFeat else [out])
            if i + 1 < self.num_D:
                x = ops.avgpool3s2(x)            # discriminator.py:28,56 (scripts/face/train_g8_512.sh: --num_D 2)
                if adaptive:
                    ref = ops.avgpool3s2(ref)
        return result


def define_G(opt):
    """Reference models/networks/__init__.py:29-39."""
    return FewShotGenerator(opt)


def define_D(opt, input_nc, ndf, n_layers_D, norm='spectralinstance', subarch='n_layers', num_D=1, getIntermFeat=False,
             stride=2, gpu_ids=()):
    """Reference models/networks/__init__.py:41-55."""
    if norm != 'spectralinstance' or subarch not in ('n_layers', 'adaptive'):
        raise NotImplementedError("only the 'spectralinstance' PatchGANs (n_layers, adaptive) are on the hot path")
    if subarch == 'adaptive' and str(getattr(opt, 'amp', 'O0')) != 'O0':
        raise NotImplementedError("--netD_subarch adaptive under --amp")
    return MultiscaleDiscriminator(opt, input_nc, ndf, n_layers_D, num_D, getIntermFeat, stride, subarch)
