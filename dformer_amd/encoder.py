"""DFormer RGB-D encoder with the reference's module tree, constructor arguments and state_dict
keys (Originofamonia/DFormer models/encoders/DFormer.py), computed by HIP kernels.

Layout: inside a stage the activations are NHWC rows in the compute dtype; the reference's
Block.forward(x [B,H,W,C], x_e [B,H,W,C/2]) -> (x, x_e) surface is kept. nn.Linear / nn.Conv2d
children are parameter containers only (their forward is never called on the hot path).
The stems / stage downsampling (BN + conv3x3 s2, DFormer.py:194-228) run on ConvS2Fn: the BN
statistics on the library's shifted-sum BN kernels, then one gather that folds the BN affine (and
the stem's GELU) into the convolution operand and one MFMA GEMM (csrc/conv.hip), reading the raw
input image and the previous stage's NHWC rows in place (no NCHW<->NHWC permute copies).
"""

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import kernels as K
from .batchnorm import bn_backward, bn_forward, collectives_on
from .functional import ATTN_PARAM_NAMES, AttentionFn, ConvFFNFn, gslot, invalidate_weights, weights_epoch
from .streams import fork, join, side_stream

_EMPTY = {}


def _empty(dev):
    t = _EMPTY.get(dev)
    if t is None:
        t = _EMPTY[dev] = torch.empty(0, device=dev)
    return t


class LayerNorm(nn.Module):
    """channels_last LayerNorm parameters (DFormer.py:21-45); compute happens inside the fused ops."""

    def __init__(self, normalized_shape, eps=1e-6, data_format="channels_last"):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(normalized_shape))
        self.bias = nn.Parameter(torch.zeros(normalized_shape))
        self.eps = eps
        self.data_format = data_format
        self.normalized_shape = (normalized_shape,)

    def forward(self, x):  # standalone use (not on the fused path)
        return F.layer_norm(x, self.normalized_shape, self.weight, self.bias, self.eps)


class MLP(nn.Module):
    """ConvFFN: LN -> fc1 -> DW3x3 + identity -> GELU -> fc2 (DFormer.py:48-67)."""

    def __init__(self, dim, mlp_ratio=4, norm_cfg=None):
        super().__init__()
        self.norm = LayerNorm(dim, eps=1e-6)
        self.fc1 = nn.Linear(dim, dim * mlp_ratio)
        self.pos = nn.Conv2d(dim * mlp_ratio, dim * mlp_ratio, 3, padding=1, groups=dim * mlp_ratio)
        self.fc2 = nn.Linear(dim * mlp_ratio, dim)
        self.act = nn.GELU()

    def fused(self, x2d, shape, rowscale, layer_scale):
        return ConvFFNFn.apply(x2d, shape, rowscale, self.norm.weight, self.norm.bias, self.fc1.weight,
                               self.fc1.bias, self.pos.weight, self.pos.bias, self.fc2.weight, self.fc2.bias,
                               layer_scale)


class Attention(nn.Module):
    """RGB-D attention (DFormer.py:70-145): conv modulation, pooled-query attention, depth branch."""

    def __init__(self, dim, num_head=8, window=7, norm_cfg=None, drop_depth=False):
        super().__init__()
        self.num_head = num_head
        self.window = window
        self.q = nn.Linear(dim, dim)
        self.q_cut = nn.Linear(dim, dim // 2)
        self.a = nn.Linear(dim, dim)
        self.l = nn.Linear(dim, dim)
        self.conv = nn.Conv2d(dim, dim, 7, padding=3, groups=dim)
        self.e_conv = nn.Conv2d(dim // 2, dim // 2, 7, padding=3, groups=dim // 2)
        self.e_fore = nn.Linear(dim // 2, dim // 2)
        self.e_back = nn.Linear(dim // 2, dim // 2)
        kin = dim * 2 if window != 0 else dim // 2 * 3
        self.proj = nn.Linear(kin, dim)
        if not drop_depth:
            self.proj_e = nn.Linear(kin, dim // 2)
        if window != 0:
            self.short_cut_linear = nn.Linear(dim // 2 * 3, dim // 2)
            self.kv = nn.Linear(dim, dim)
            self.pool = nn.AdaptiveAvgPool2d(output_size=(7, 7))
        self.act = nn.GELU()
        self.norm = LayerNorm(dim, eps=1e-6)
        self.norm_e = LayerNorm(dim // 2, eps=1e-6)
        self.drop_depth = drop_depth

    def fused_params(self, ls1, ls1e):
        e = _empty(self.q.weight.device)
        w = self.window != 0
        d = not self.drop_depth
        vals = dict(n_w=self.norm.weight, n_b=self.norm.bias, ne_w=self.norm_e.weight, ne_b=self.norm_e.bias,
                    wq=self.q.weight, bq=self.q.bias, wqc=self.q_cut.weight, bqc=self.q_cut.bias, wl=self.l.weight,
                    bl=self.l.bias, wconv=self.conv.weight, bconv=self.conv.bias, wa=self.a.weight, ba=self.a.bias,
                    wef=self.e_fore.weight, bef=self.e_fore.bias, wec=self.e_conv.weight, bec=self.e_conv.bias,
                    web=self.e_back.weight, beb=self.e_back.bias,
                    wkv=self.kv.weight if w else e, bkv=self.kv.bias if w else e,
                    wsc=self.short_cut_linear.weight if w else e, bsc=self.short_cut_linear.bias if w else e,
                    wp=self.proj.weight, bp=self.proj.bias,
                    wpe=self.proj_e.weight if d else e, bpe=self.proj_e.bias if d else e,
                    ls1=ls1, ls1e=ls1e if ls1e is not None else e)
        return [vals[n] for n in ATTN_PARAM_NAMES]


def _drop_path_scale(B, drop_prob, training, dev):
    """mmcv DropPath as a per-sample row scale: floor(keep + U[0,1)) / keep, or None."""
    if drop_prob == 0.0 or not training:
        return None
    keep = 1.0 - drop_prob
    return (keep + torch.rand(B, device=dev)).floor_().div_(keep)


class Block(nn.Module):
    """DFormer Block (DFormer.py:147-181): x + DropPath(ls1 * attn), + DropPath(ls2 * MLP), both branches."""

    def __init__(self, index, dim, num_head, norm_cfg=None, mlp_ratio=4.0, block_index=0, last_block_index=50,
                 window=7, dropout_layer=None, drop_depth=False):
        super().__init__()
        self.index = index
        layer_scale_init_value = 1e-6
        if block_index > last_block_index:
            window = 0
        self.attn = Attention(dim, num_head, window=window, norm_cfg=norm_cfg, drop_depth=drop_depth)
        self.mlp = MLP(dim, int(mlp_ratio), norm_cfg=norm_cfg)
        self.drop_prob = float(dropout_layer.get("drop_prob", 0.0)) if dropout_layer else 0.0
        self.layer_scale_1 = nn.Parameter(layer_scale_init_value * torch.ones(dim))
        self.layer_scale_2 = nn.Parameter(layer_scale_init_value * torch.ones(dim))
        if not drop_depth:
            self.layer_scale_1_e = nn.Parameter(layer_scale_init_value * torch.ones(dim // 2))
            self.layer_scale_2_e = nn.Parameter(layer_scale_init_value * torch.ones(dim // 2))
            self.mlp_e2 = MLP(dim // 2, int(mlp_ratio))
        self.drop_depth = drop_depth
        self.drop_path_masks = None  # tests may inject the 4 per-sample keep masks (mmcv call order)
        self._row_scales = None  # [4, B] DropPath scales drawn for the whole backbone by DFormer.forward

    def forward(self, x, x_e):
        if not x.is_cuda:
            raise RuntimeError("dformer_amd runs on the HIP library only (tensors must be on the GPU)")
        B, H, W, C = x.shape
        shape = (B, H, W)
        xr = x.reshape(B * H * W, C)
        xer = x_e.reshape(B * H * W, C // 2)
        if self.drop_path_masks is not None and self.training and self.drop_prob > 0:
            keep = 1.0 - self.drop_prob
            rs = [m.to(device=x.device, dtype=torch.float32) / keep for m in self.drop_path_masks]
        elif self._row_scales is not None:
            rs = list(self._row_scales.unbind(0))
            self._row_scales = None
        else:
            rs = [_drop_path_scale(B, self.drop_prob, self.training, x.device) for _ in range(4)]
        ls1e = self.layer_scale_1_e if not self.drop_depth else None
        st = getattr(self, "stage", "s?")
        K.TAG = st + ".attn"
        x1, xe1 = AttentionFn.apply(xr, xer, shape, self.attn.num_head, self.attn.window, self.drop_depth, rs[0],
                                    rs[2], *self.attn.fused_params(self.layer_scale_1, ls1e))
        if self.drop_depth:
            K.TAG = st + ".mlp"
            x2 = self.mlp.fused(x1, shape, rs[1], self.layer_scale_2)
            return x2.view(B, H, W, C), xe1.view(B, H, W, C // 2)  # DFormer.py:177-181: e_back's output
        # the RGB and depth ConvFFNs are independent: the RGB one runs on a side stream (and so does its
        # backward: autograd replays a node on its forward's stream) while the depth one runs on the
        # step's stream; the overlap fills the GPU at the late stages where each kernel alone is
        # latency-bound. (RGB on the side: 491.8 / 491.0 vs 488.2 / 487.8 images/s with the depth
        # ConvFFN there — the side stream's kernels get the smaller share of the CUs, and the join waited
        # 2.3 ms per step on the depth ConvFFN finishing after the RGB one, profiles/r06_queue_analysis.txt)
        side = side_stream(x.device, "ffn")
        with fork(side, reads=(x1,)):
            K.TAG = st + ".mlp"
            x2 = self.mlp.fused(x1, shape, rs[1], self.layer_scale_2)
        K.TAG = st + ".mlp_e2"
        xe2 = self.mlp_e2.fused(xe1, shape, rs[3], self.layer_scale_2_e)
        join(side, made=(x2,))
        return x2.view(B, H, W, C), xe2.view(B, H, W, C // 2)


def _bn(c, syncbn):
    return nn.SyncBatchNorm(c) if syncbn else nn.BatchNorm2d(c)


class BNRowsFn(torch.autograd.Function):
    """BatchNorm2d / SyncBatchNorm (DFormer.py:219-228 stems and downsample layers) on a
    channels-last NCHW tensor, computed as [B*H*W, C] rows by the library's BN kernels: batch
    statistics + running-stat update in training (all-reduced for SyncBN), running stats in eval."""

    @staticmethod
    def forward(ctx, x, gamma, beta, bn, sync):
        B, C, H, W = x.shape
        xr = x.permute(0, 2, 3, 1).contiguous().view(-1, C)
        mean, rstd, count = bn_forward(xr, bn, sync)
        y = K.bn_apply(xr, mean, rstd, gamma, beta)
        ctx.save_for_backward(xr, mean, rstd, gamma)
        ctx.sync, ctx.count, ctx.shape, ctx.bn = sync, count, (B, C, H, W), bn
        ctx.training = bn.training
        return y.view(B, H, W, C).permute(0, 3, 1, 2)

    @staticmethod
    def backward(ctx, dy):
        K.TAG = "down.bwd"
        xr, mean, rstd, gamma = ctx.saved_tensors
        B, C, H, W = ctx.shape
        dyr = dy.permute(0, 2, 3, 1).contiguous().view(-1, C)
        dx, dgamma, dbeta = bn_backward(dyr, xr, (mean, rstd, ctx.count), gamma, ctx.bn, ctx.sync, ctx.training)
        return dx.view(B, H, W, C).permute(0, 3, 1, 2), dgamma, dbeta, None, None


class ConvS2Fn(torch.autograd.Function):
    """nn.Conv2d(cin, cout, 3, stride 2, pad 1) [preceded by BatchNorm / SyncBatchNorm [+ GELU]]
    (DFormer.py:194-228: stem conv -> BN -> GELU -> conv; stage i>0: BN -> conv) on the library's
    kernels: the BN statistics over the input rows, then ONE gather that applies the BN affine and
    GELU on the fly (csrc/conv.hip) and ONE MFMA GEMM with the conv bias in its epilogue. x is any
    NCHW-logical tensor (raw image, the depth-channel view, or the previous stage's NHWC rows);
    returns NHWC rows [B*Ho*Wo, cout] in the compute dtype. Backward: weight / bias gradients
    from the saved gathered operand, input gradient by the transposed GEMM + deterministic
    col2im with GELU' recomputed, then the BN backward."""

    @staticmethod
    def forward(ctx, x, weight, bias, bn_w, bn_b, bn, sync, gelu, dt):
        B, C, H, W = x.shape
        cout = weight.shape[0]
        kp = K.conv3s2_kp(C)
        aff = None
        count = None
        xr = None
        if bn is not None:
            xr = x.permute(0, 2, 3, 1).reshape(B * H * W, C)  # the NHWC rows (a view for channels-last x)
            mean, rstd, count = bn_forward(xr, bn, sync)
            aff = (mean, rstd, bn_w.detach(), bn_b.detach())
        cols = K.conv3s2_im2col(x, dt, bn=aff, gelu=gelu)
        wp = K.conv3_weight_pack(weight.detach(), dt, kp)
        y = K.linear(cols, wp, bias.detach())
        ctx.shape, ctx.cin, ctx.sync, ctx.gelu, ctx.count = (B, H, W), C, sync, gelu, count
        ctx.has_bn = bn is not None
        ctx.bn = bn
        ctx.training = bn is not None and bn.training
        ctx.x_dtype = x.dtype
        ctx.tag = K.TAG
        ctx.save_for_backward(cols, wp, weight, bias, xr if xr is not None else x.new_empty(0),
                              *(aff if aff is not None else ()))
        return y

    @staticmethod
    def backward(ctx, dy):
        K.TAG = ctx.tag + ".bwd"
        cols, wp, weight, bias, xr, *aff = ctx.saved_tensors
        dy = dy.contiguous()
        cin = ctx.cin
        dwp, db = K.linear_wgrad(dy, cols, bias_grad=True, bias_out=gslot(bias))
        dw = K.conv3_weight_unpack(dwp, cin, dw=gslot(weight))
        dx = dgamma = dbeta = None
        if not ctx.has_bn:
            if ctx.needs_input_grad[0]:  # gradient w.r.t. the image (parity tests); not on the training path
                dx = K.conv3s2_col2im_nchw(K.linear_dgrad(dy, wp), ctx.shape, cin, ctx.x_dtype)
        elif ctx.needs_input_grad[0] or ctx.needs_input_grad[3] or ctx.needs_input_grad[4]:
            dcols = K.linear_dgrad(dy, wp)
            mean, rstd, gamma, beta = aff
            dz = K.conv3s2_col2im(dcols, ctx.shape, cin, x=xr, bn=aff if ctx.gelu else None, gelu=ctx.gelu)
            dx, dgamma, dbeta = bn_backward(dz, xr, (mean, rstd, ctx.count), gamma, ctx.bn, ctx.sync, ctx.training,
                                            need_dx=ctx.needs_input_grad[0])
            if dx is not None:
                B, H, W = ctx.shape
                dx = dx.view(B, H, W, cin).permute(0, 3, 1, 2)
        return dx, dw, db, dgamma, dbeta, None, None, None, None


# The stem / downsample layers run natively: 3x3 stride-2 convs as gather + MFMA GEMM with their
# BatchNorms (+ GELU) folded into the gather (ConvS2Fn), the stem's last BN on BNRowsFn. There is no
# vendor-convolution path.


def _run_downsample_native(seq, x, dt):
    """The reference's downsample nn.Sequential (stem: Conv, BN, GELU, Conv, BN; stage: BN, Conv)
    on ConvS2Fn / BNRowsFn. Returns the NCHW-logical view of channels-last rows."""
    mods = list(seq)
    i, pend_bn, pend_gelu = 0, None, False
    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.modules.batchnorm._BatchNorm):
            if i == len(mods) - 1:  # trailing BN of the stem: applied to the conv output rows
                x = BNRowsFn.apply(x, m.weight, m.bias, m, isinstance(m, nn.SyncBatchNorm))
            else:
                pend_bn = m
        elif isinstance(m, nn.GELU):
            assert pend_bn is not None
            pend_gelu = True
        else:
            assert isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3) and m.stride == (2, 2) and m.padding == (1, 1)
            B, _, H, W = x.shape
            bn = pend_bn
            y = ConvS2Fn.apply(x, m.weight, m.bias, bn.weight if bn is not None else None,
                               bn.bias if bn is not None else None, bn, isinstance(bn, nn.SyncBatchNorm), pend_gelu,
                               dt)
            Ho, Wo = (H + 1) // 2, (W + 1) // 2
            x = y.view(B, Ho, Wo, m.out_channels).permute(0, 3, 1, 2)
            pend_bn, pend_gelu = None, False
        i += 1
    return x


class DFormer(nn.Module):
    """DFormer backbone (DFormer.py:184-305). forward(x, x_e) -> (outs[4] NCHW views, None) like the
    reference; outs are channels-last buffers in the compute dtype."""

    def __init__(self, in_channels=4, depths=(2, 2, 8, 2), dims=(32, 64, 128, 256), out_indices=(0, 1, 2, 3),
                 windows=(7, 7, 7, 7), norm_cfg=None, mlp_ratios=(8, 8, 4, 4), num_heads=(2, 4, 10, 16),
                 last_block=(50, 50, 50, 50), drop_path_rate=0.1, init_cfg=None):
        super().__init__()
        syncbn = bool(norm_cfg) and norm_cfg.get("type") == "SyncBN" and collectives_on()
        self.depths = depths
        self.dims = dims
        self.mlp_ratios = mlp_ratios
        self.out_indices = out_indices
        self.compute_dtype = torch.float32
        self.downsample_layers = nn.ModuleList()
        self.downsample_layers.append(nn.Sequential(
            nn.Conv2d(3, dims[0] // 2, 3, 2, 1), nn.BatchNorm2d(dims[0] // 2), nn.GELU(),
            nn.Conv2d(dims[0] // 2, dims[0], 3, 2, 1), nn.BatchNorm2d(dims[0])))
        self._register_depth_front()
        self.downsample_layers_e = nn.ModuleList()
        self.downsample_layers_e.append(nn.Sequential(
            nn.Conv2d(1, dims[0] // 4, 3, 2, 1), nn.BatchNorm2d(dims[0] // 4), nn.GELU(),
            nn.Conv2d(dims[0] // 4, dims[0] // 2, 3, 2, 1), nn.BatchNorm2d(dims[0] // 2)))
        for i in range(len(dims) - 1):
            self.downsample_layers.append(nn.Sequential(_bn(dims[i], syncbn),
                                                        nn.Conv2d(dims[i], dims[i + 1], 3, 2, 1)))
            self.downsample_layers_e.append(nn.Sequential(_bn(dims[i] // 2, syncbn),
                                                          nn.Conv2d(dims[i] // 2, dims[i + 1] // 2, 3, 2, 1)))
        self.stages = nn.ModuleList()
        dp_rates = [x.item() for x in torch.linspace(0, drop_path_rate, sum(depths))]
        cur = 0
        for i in range(len(dims)):
            self.stages.append(nn.Sequential(*[
                Block(index=cur + j, dim=dims[i], window=windows[i],
                      dropout_layer=dict(type="DropPath", drop_prob=dp_rates[cur + j]), num_head=num_heads[i],
                      norm_cfg=norm_cfg, block_index=depths[i] - j, last_block_index=last_block[i],
                      mlp_ratio=mlp_ratios[i], drop_depth=((i == 3) & (j == depths[i] - 1)))
                for j in range(depths[i])]))
            for blk in self.stages[-1]:
                blk.stage = f"s{i}"
            cur += depths[i]

    def _register_depth_front(self):
        """The children the reference registers between the RGB stem and the depth stem."""
        # unused by the reference forward (DFormer.py:202-203, 287-291); kept for state_dict parity
        self.stem_e_fc1 = nn.Linear(360, 640)
        self.stem_e_fc2 = nn.Linear(1, 480)
        for p in (self.stem_e_fc1.weight, self.stem_e_fc1.bias, self.stem_e_fc2.weight, self.stem_e_fc2.bias):
            p.requires_grad_(False)  # never used: excluded from gradients (and DDP buckets)

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        invalidate_weights()
        return r

    def _draw_drop_path(self, B, dev):
        """mmcv DropPath scales floor(keep + U[0,1)) / keep for all four DropPath calls of every
        Block, drawn by one RNG launch for the whole backbone instead of four per Block."""
        blocks = [b for st in self.stages for b in st]
        if not self.training or all(b.drop_prob == 0.0 for b in blocks):
            return
        keep = getattr(self, "_keep", None)
        if keep is None or keep.device != dev:
            keep = self._keep = torch.tensor([1.0 - b.drop_prob for b in blocks], device=dev).view(-1, 1, 1)
        rs = (keep + torch.rand(len(blocks), 4, B, device=dev)).floor_().div_(keep)
        for b, r in zip(blocks, rs.unbind(0)):
            b._row_scales = r if b.drop_prob > 0 else None

    def _downsample(self, i, x, e):
        if not x.is_cuda:
            raise RuntimeError("dformer_amd runs on the HIP library only (tensors must be on the GPU)")
        dt = self.compute_dtype
        seq_e = self.downsample_layers_e[i]
        if any(isinstance(m, nn.SyncBatchNorm) for m in seq_e):
            return (_run_downsample_native(self.downsample_layers[i], x, dt),
                    _run_downsample_native(seq_e, e, dt))
        # the two branches' stems / downsamples are independent: the depth one runs on the side
        # stream (its backward too) next to the RGB one on the step's stream (same box, alternated:
        # 506.2 / 509.8 vs 503.3 / 500.2 images/s; SyncBN keeps both on the step's stream)
        side = side_stream(x.device, "ffn")
        with fork(side, reads=(e,)):
            e2 = _run_downsample_native(seq_e, e, dt)
        x2 = _run_downsample_native(self.downsample_layers[i], x, dt)
        join(side, made=(e2,))
        return x2, e2

    def forward(self, x, x_e):
        if x_e is None:
            x_e = x
        if x.dim() == 3:
            x = x.unsqueeze(0)
        if x_e.dim() == 3:
            x_e = x_e.unsqueeze(2)
        return self._run_stages(x, x_e[:, 0:1]), None

    def _run_stages(self, x, x_e):
        """The four stages (DFormer.py:293-304, 445-456) on the image x and the depth plane x_e [B, 1, H, W]."""
        dt = self.compute_dtype
        self._draw_drop_path(x.shape[0], x.device)
        outs = []
        for i in range(4):
            K.TAG = f"s{i}.down"
            x, x_e = self._downsample(i, x, x_e)
            xh = x.permute(0, 2, 3, 1).to(dt).contiguous()
            eh = x_e.permute(0, 2, 3, 1).to(dt).contiguous()
            for blk in self.stages[i]:
                xh, eh = blk(xh, eh)
            x = xh.permute(0, 3, 1, 2)  # NCHW view of the channels-last buffer
            x_e = eh.permute(0, 3, 1, 2)
            outs.append(x)
        return outs


class LaserExpandFn(torch.autograd.Function):
    """The collapsed Attention1Dto2D (DFormer.py:308-339) on csrc/laser.hip: scans [B, N] and the folded
    (alpha [L, Hh], g [Hh], c [1]) -> the depth plane [B, Hout, L], float32, constant along Hout.
    Backward: dalpha, dg, dc by fixed-order sums. The scan is input data: it gets no gradient."""

    @staticmethod
    def forward(ctx, scan, alpha, g, c, hout):
        save = any(ctx.needs_input_grad[1:4])
        plane, _, mean, var = K.laser_expand_fwd(scan, alpha, g, c, hout, save=save)
        if save:
            ctx.save_for_backward(g, mean, var)
        return plane

    @staticmethod
    def backward(ctx, dplane):
        K.TAG = "laser.bwd"
        g, mean, var = ctx.saved_tensors
        _, dalpha, dg, dc = K.laser_expand_bwd(dplane.contiguous(), g, mean, var)
        return None, dalpha, dg, dc, None


class _MHAParams(nn.Module):
    """The parameters of an nn.MultiheadAttention(embed_dim, num_heads) under its state-dict keys
    (in_proj_weight, in_proj_bias, out_proj.*), initialised like it. A container: it has no forward."""

    def __init__(self, embed_dim):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * embed_dim))
        self.out_proj = nn.Linear(embed_dim, embed_dim)
        nn.init.xavier_uniform_(self.in_proj_weight)
        nn.init.zeros_(self.out_proj.bias)


class Attention1Dto2D(nn.Module):
    """The laser-scan expansion of DFormerTrav (DFormer.py:308-339), with the reference's constructor
    and state-dict keys. forward(x [B, 1, N]) -> [B, 1, output_len, mid_len] float32.

    What the reference computes collapses: attn2 attends over one key, so its softmax is
    1 and the plane is constant along output_len (query2 and attn2's Q / K projections have no effect);
    input_proj is Linear(1, E), so attn1's scores are alpha[l, h] * x[j] + const. fold() forms
    (alpha, g, c) from the parameters by differentiable tensor ops in float64; LaserExpandFn does the
    B * L * Hh * N exponentials and the one plane write."""

    def __init__(self, input_len=360, mid_len=640, output_len=480, embed_dim=64, num_heads=4):
        super().__init__()
        if embed_dim % num_heads != 0 or not 1 <= num_heads <= 8:
            raise ValueError(f"Attention1Dto2D: embed_dim {embed_dim} / num_heads {num_heads} (1..8 heads)")
        if input_len > K.LASER_MAX_N:
            raise ValueError(f"Attention1Dto2D: input_len {input_len} exceeds the kernel's {K.LASER_MAX_N} ranges")
        self.input_len = input_len  # documentation only in the reference: any scan length runs
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.mid_len = mid_len
        self.output_len = output_len
        self.input_proj = nn.Linear(1, embed_dim)
        self.query1 = nn.Parameter(torch.randn(mid_len, embed_dim))
        self.attn1 = _MHAParams(embed_dim)
        self.query2 = nn.Parameter(torch.randn(output_len, embed_dim))
        self.attn2 = _MHAParams(embed_dim)
        self.output_proj = nn.Linear(embed_dim, 1)
        self._folded = None

    def fold(self):
        """(alpha [L, Hh], g [Hh], c [1]) float32 from the parameters, differentiable:
        alpha[l, h] = (W_q query1[l] + b_q)_h . (W_k w_in)_h / sqrt(dh);  u = W_o1^T W_v2^T W_o2^T w_out;
        g[h] = u_h . (W_v w_in)_h;  c = u . (W_v b_in + b_v) + w_out . (W_o2 (W_v2 b_o1 + b_v2) + b_o2) + b_out.
        The K third of attn1.in_proj_bias cancels in the softmax and query2 / attn2's Q and K thirds are
        multiplied by a softmax over one key: their gradients are exact zeros, as in the reference."""
        E, Hh = self.embed_dim, self.num_heads
        dh = E // Hh
        d = torch.float64
        w_in, b_in = self.input_proj.weight.to(d)[:, 0], self.input_proj.bias.to(d)
        w1, b1 = self.attn1.in_proj_weight.to(d), self.attn1.in_proj_bias.to(d)
        w2, b2 = self.attn2.in_proj_weight.to(d), self.attn2.in_proj_bias.to(d)
        wq, wk, wv, bq, bv = w1[:E], w1[E:2 * E], w1[2 * E:], b1[:E], b1[2 * E:]
        wv2, bv2 = w2[2 * E:], b2[2 * E:]
        wo1, bo1 = self.attn1.out_proj.weight.to(d), self.attn1.out_proj.bias.to(d)
        wo2, bo2 = self.attn2.out_proj.weight.to(d), self.attn2.out_proj.bias.to(d)
        w_out, b_out = self.output_proj.weight.to(d)[0], self.output_proj.bias.to(d)
        q = self.query1.to(d) @ wq.t() + bq
        alpha = (q.view(-1, Hh, dh) * (wk @ w_in).view(Hh, dh)).sum(-1) / dh ** 0.5
        u = wo1.t() @ (wv2.t() @ (wo2.t() @ w_out))
        g = (u.view(Hh, dh) * (wv @ w_in).view(Hh, dh)).sum(-1)
        c = u @ (wv @ b_in + bv) + w_out @ (wo2 @ (wv2 @ bo1 + bv2) + bo2) + b_out
        c = c + 0.0 * self.query2.to(d).sum()  # no effect on the output: an exact-zero gradient, not None
        return alpha.float().contiguous(), g.float().contiguous(), c.float().reshape(1)

    def folded(self):
        """fold(), cached across no-grad calls until invalidate_weights() (load_state_dict, optimizer step)."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return self.fold()
        key = (weights_epoch(), self.query1.device, self.query1.data_ptr())
        if self._folded is None or self._folded[0] != key:
            with torch.no_grad():
                self._folded = (key, self.fold())
        return self._folded[1]

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("dformer_amd runs on the HIP library only (tensors must be on the GPU)")
        B = x.shape[0]
        scan = x.reshape(B, -1).float().contiguous()  # DFormer.py:325-326: [B, 1, N] -> N ranges per image
        alpha, g, c = self.folded()
        K.TAG = "laser"
        plane = LaserExpandFn.apply(scan, alpha, g, c, self.output_len)
        return plane.view(B, 1, self.output_len, self.mid_len)


class DFormerTrav(DFormer):
    """The traversability backbone (DFormer.py:342-457): DFormer whose depth plane is the expansion of a
    laser scan. Children in the reference's order (downsample_layers, attn_expand_e, downsample_layers_e,
    stages), no stem_e_fc*; forward(x, x_e) takes the scan x_e [B, 1, N] and returns the list outs.
    expand = (input_len, mid_len, output_len) of the expansion (the reference's are fixed at 360, 640, 480)."""

    scan_input = True  # modal_x is a scan: it cannot be resized, cropped or flipped (evaluate.py)

    def __init__(self, depths=(2, 2, 8, 2), dims=(32, 64, 128, 256), out_indices=(0, 1, 2, 3), windows=(7, 7, 7, 7),
                 norm_cfg=None, mlp_ratios=(8, 8, 4, 4), num_heads=(2, 4, 10, 16), last_block=(50, 50, 50, 50),
                 drop_path_rate=0.1, init_cfg=None, expand=(360, 640, 480)):
        self.expand = tuple(expand)  # read by _register_depth_front during DFormer.__init__
        super().__init__(depths=depths, dims=dims, out_indices=out_indices, windows=windows, norm_cfg=norm_cfg,
                         mlp_ratios=mlp_ratios, num_heads=num_heads, last_block=last_block,
                         drop_path_rate=drop_path_rate, init_cfg=init_cfg)

    def _register_depth_front(self):
        n, mid, out = self.expand
        self.attn_expand_e = Attention1Dto2D(input_len=n, mid_len=mid, output_len=out, embed_dim=64, num_heads=4)

    def forward(self, x, x_e):
        if x_e is None:
            raise ValueError("DFormerTrav: the laser scan x_e [B, 1, N] is required")
        if x.dim() == 3:
            x = x.unsqueeze(0)
        elif x.dim() == 5:  # DFormer.py:440-442
            x = x.reshape(-1, *x.shape[2:])
        B = x.shape[0]
        if x_e.numel() % B != 0:
            raise ValueError(f"DFormerTrav: scans {tuple(x_e.shape)} do not match {B} images")
        exp = self.attn_expand_e
        if (exp.output_len, exp.mid_len) != tuple(x.shape[-2:]):
            raise ValueError(f"DFormerTrav: the expansion's plane {exp.output_len} x {exp.mid_len} does not match "
                             f"the image {tuple(x.shape[-2:])}")
        return self._run_stages(x, exp(x_e.reshape(B, 1, -1)))


def get_DFormerTrav(pretrained=False, drop_path_rate=0.1, **kwargs):
    return DFormerTrav(dims=[64, 128, 256, 512], mlp_ratios=[8, 8, 4, 4], depths=[3, 3, 12, 2],
                       num_heads=[1, 2, 4, 8], windows=[0, 7, 7, 7], drop_path_rate=drop_path_rate, **kwargs)


def DFormer_Tiny(pretrained=False, **kwargs):
    return DFormer(dims=[32, 64, 128, 256], mlp_ratios=[8, 8, 4, 4], depths=[3, 3, 5, 2], num_heads=[1, 2, 4, 8],
                   windows=[0, 7, 7, 7], **kwargs)


def DFormer_Small(pretrained=False, **kwargs):
    return DFormer(dims=[64, 128, 256, 512], mlp_ratios=[8, 8, 4, 4], depths=[2, 2, 4, 2], num_heads=[1, 2, 4, 8],
                   windows=[0, 7, 7, 7], **kwargs)


def DFormer_Base(pretrained=False, drop_path_rate=0.1, **kwargs):
    return DFormer(dims=[64, 128, 256, 512], mlp_ratios=[8, 8, 4, 4], depths=[3, 3, 12, 2], num_heads=[1, 2, 4, 8],
                   windows=[0, 7, 7, 7], drop_path_rate=drop_path_rate, **kwargs)


def DFormer_Large(pretrained=False, drop_path_rate=0.1, **kwargs):
    return DFormer(dims=[96, 192, 288, 576], mlp_ratios=[8, 8, 4, 4], depths=[3, 3, 12, 2], num_heads=[1, 2, 4, 8],
                   windows=[0, 7, 7, 7], drop_path_rate=drop_path_rate, **kwargs)
