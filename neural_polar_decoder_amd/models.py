"""convNet decoder -- drop-in for models.convNet (models.py:691-772).

Same modules and parameter names as the reference (so ``load_state_dict`` of a reference checkpoint
works); ``decode``/``forward`` run the whole network through libnpd's MFMA kernels
(npd_conv_forward): implicit-GEMM dilated Conv1d + GELU (+ residual) layers, FC GEMMs with fused
bias/GELU, LayerNorm + sign.

XFormerEndToEndGPT -- drop-in for models.XFormerEndToEndGPT (models.py:340-423, ``--model gpt``): the same module
tree; ``decode`` runs the successive decode in one launch of npd_gpt_decode.

XFormerEndToEndDecoder / XFormerEndToEndEncoder -- drop-ins for the reference's ``--model decoder`` (models.py:599-654)
and ``--model encoder`` (models.py:662-686): ``decode`` runs in one launch of npd_xfdec_decode / npd_xfenc_forward.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch
import torch.nn as nn

from . import _lib


class convNet(nn.Module):
    """models.convNet.  ``precision`` (keyword, not in the reference): "fp32" (default; exact fp32 FMA chains on
    v_mfma_f32_32x32x2_f32) or "fp16x3" (the conv layers with cin > 1 and the three Linear layers on v_mfma_f32_32x32x16_f16
    with hi + lo fp16 operands, three products per multiply, fp32 accumulation; layer 0, GELU, residuals and
    LayerNorm stay fp32)."""

    PRECISIONS = {"fp32": 0, "fp16x3": 3}

    def __init__(self, config, precision="fp32"):
        super().__init__()
        if precision not in self.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(self.PRECISIONS)}")
        self.precision = precision
        self.hidden_dim = config.embed_dim
        self.input_len = config.max_len
        self.output_len = config.N
        bias = not getattr(config, "dont_use_bias", False)
        self.use_bias = bias
        k, p = 7, 3
        h, e = self.hidden_dim // 2, self.hidden_dim
        self.kernel, self.padding = k, p
        self.layers1 = nn.Sequential(nn.Conv1d(1, h, k, padding=p, bias=bias), nn.GELU(),
                                     nn.Conv1d(h, h, k, padding=2 * p, dilation=2, bias=bias), nn.GELU())
        self.layers2 = nn.Sequential(nn.Conv1d(h, h, k, padding=4 * p, dilation=4, bias=bias), nn.GELU(),
                                     nn.Conv1d(h, h, k, padding=p, bias=bias), nn.GELU())
        self.layers3 = nn.Sequential(nn.Conv1d(h, h, k, padding=2 * p, dilation=2, bias=bias), nn.GELU(),
                                     nn.Conv1d(h, h, k, padding=4 * p, dilation=4, bias=bias), nn.GELU())
        self.layers4 = nn.Sequential(nn.Conv1d(h, h, k, padding=p, bias=bias), nn.GELU(),
                                     nn.Conv1d(h, h, k, padding=2 * p, dilation=2, bias=bias), nn.GELU())
        self.layers5 = nn.Sequential(nn.Conv1d(h, e, k, padding=4 * p, dilation=4, bias=bias), nn.GELU(),
                                     nn.Conv1d(e, e, k, padding=p, bias=bias), nn.GELU())
        n = self.output_len
        self.layersFin = nn.Sequential(nn.Linear(e * n, 4 * n), nn.GELU(), nn.Linear(4 * n, n), nn.GELU(),
                                       nn.Linear(n, n))
        self.layer_norm = nn.LayerNorm(n, eps=1e-6)
        self.dropout = nn.Dropout(getattr(config, "dropout", 0.0))
        self._handle = None
        self._hkey = None

    # ------------------------------------------------------------------ fused path
    def _packed(self) -> np.ndarray:
        parts = []
        convs = [self.layers1[0], self.layers1[2], self.layers2[0], self.layers2[2], self.layers3[0], self.layers3[2],
                 self.layers4[0], self.layers4[2], self.layers5[0], self.layers5[2]]
        for c in convs:
            parts.append(c.weight.detach().float().cpu().numpy().ravel())
            b = c.bias.detach().float().cpu().numpy() if c.bias is not None else np.zeros(c.out_channels, np.float32)
            parts.append(b.ravel())
        for li in (0, 2, 4):
            parts.append(self.layersFin[li].weight.detach().float().cpu().numpy().ravel())
            parts.append(self.layersFin[li].bias.detach().float().cpu().numpy().ravel())
        parts.append(self.layer_norm.weight.detach().float().cpu().numpy().ravel())
        parts.append(self.layer_norm.bias.detach().float().cpu().numpy().ravel())
        return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)

    def _get_handle(self, device):
        key = (str(device), self.precision, tuple(p._version for p in self.parameters()),
               tuple(p.data_ptr() for p in self.parameters()))
        if self._handle is None or self._hkey != key:
            W = self._packed()
            out = ctypes.c_void_p()
            L = _lib.load()
            with torch.cuda.device(device):
                _lib.check(L.npd_conv_create(int(self.output_len), int(self.hidden_dim), W.ctypes.data_as(ctypes.c_void_p),
                                             int(W.size), self.PRECISIONS[self.precision], ctypes.byref(out)),
                           "npd_conv_create")
            if self._handle is not None:
                L.npd_conv_destroy(self._handle)
            self._handle, self._hkey = out, key
        return self._handle

    def __del__(self):
        try:
            if self._handle is not None:
                _lib.load().npd_conv_destroy(self._handle)
        except Exception:
            pass

    def tap_shape(self, tap: int, B: int):
        """Shape of activation ``tap`` (npd_conv_forward_tap): conv layers 0 .. 9 channels-first, then FC0 / FC1 / FC2."""
        n, h, e = self.output_len, self.hidden_dim // 2, self.hidden_dim
        if not 0 <= tap <= 12:
            raise ValueError("tap must be 0 .. 12")
        if tap < 10:
            return (B, e if tap >= 8 else h, n)
        return (B, 4 * n if tap == 10 else n)

    def logits(self, noisy_enc: torch.Tensor, want_decisions=True, want_input4=False, tap=None):
        """(logits, decisions); with ``want_input4`` also the activation after conv layer 5, with ``tap`` = 0 .. 12
        instead any one intermediate activation (conv layer ``tap``'s output, (B, cout, N); 10, 11, 12: the three
        Linear outputs, the last before LayerNorm) as a third value."""
        if tap is not None and want_input4:
            raise ValueError("ask for input4 or for a tap, not both")
        if want_input4:
            tap = 5
        if self.training:
            raise _lib.NpdError("the fused convNet path is inference-only (eval mode)")
        y = _lib.f32c(_lib.stage(noisy_enc, "noisy_enc"))
        B = y.shape[0]
        if y.shape[1] != self.output_len:
            raise ValueError("input length must equal config.N (= max_len)")
        h = self._get_handle(y.device)
        L = _lib.load()
        wsb = L.npd_conv_workspace_bytes(h, B)
        ws = torch.empty(max(int(wsb), 1), dtype=torch.uint8, device=y.device)
        lg = torch.empty(B, self.output_len, dtype=torch.float32, device=y.device)
        dec = torch.empty_like(lg) if want_decisions else None
        in4 = torch.empty(self.tap_shape(tap, B), dtype=torch.float32, device=y.device) if tap is not None else None
        _lib.check(L.npd_conv_forward_tap(h, _lib.ptr(y), _lib.ptr(lg), _lib.ptr(dec), 5 if tap is None else int(tap),
                                          _lib.ptr(in4), _lib.ptr(ws), B, _lib.stream_of(y.device)),
                   "npd_conv_forward")
        if tap is not None:
            return _lib.home(lg, noisy_enc), _lib.home(dec, noisy_enc), _lib.home(in4, noisy_enc)
        return _lib.home(lg, noisy_enc), _lib.home(dec, noisy_enc)

    # ------------------------------------------------------------------ training (models.py:742-767, run_models.py:826-915)
    def _convs(self):
        return [self.layers1[0], self.layers1[2], self.layers2[0], self.layers2[2], self.layers3[0], self.layers3[2],
                self.layers4[0], self.layers4[2], self.layers5[0], self.layers5[2]]

    def train_reason(self, y=None):
        """Why forward() in training mode refuses this net (None: it runs on the fused training kernels,
        npd_conv_train_forward / _backward) -- checked before any GPU call."""
        if self.precision != "fp32":
            return f"fused conv training runs fp32; the fp16x3 split is a follow-up, got precision {self.precision!r}"
        if next(self.parameters()).device.type != "cuda":
            return "fused conv training needs the net on the GPU: libnpd has no CPU path"
        if y is not None and getattr(y, "requires_grad", False):
            return "fused conv training returns no gradient for y: y.requires_grad must be False"
        n, e = self.output_len, self.hidden_dim
        if not (64 <= n <= 1024 and n % 64 == 0) or self.input_len != n:
            return f"fused conv training needs N = max_len a multiple of 64 in [64, 1024], got N {n}, max_len {self.input_len}"
        if not (16 <= e <= 448 and e % 16 == 0):
            return f"fused conv training needs embed_dim a multiple of 16 in [16, 448], got {e}"
        return None

    def train_supported(self, y=None) -> bool:
        """True when forward() in training mode runs on the fused training kernels (no GPU call)."""
        return self.train_reason(y) is None

    def train_logits(self, noisy_enc, drop_mult=None, want_input4=False):
        """Training-mode logits (B, N) with a grad_fn: one fused forward now, the fused backward when .backward() runs.
        With ``want_input4`` also a detached (B, embed/2, N) copy of the activation after layers3 + residual.
        ``drop_mult`` (B, N) of 0 or 1 / (1 - p) replaces the Dropout layer's own draw; None draws it from torch's
        generator on the net's device as bernoulli(1 - p) / (1 - p) when ``self.dropout.p > 0`` -- the same distribution
        as nn.Dropout, not its random stream bit for bit."""
        why = self.train_reason(noisy_enc)
        if why is not None:
            raise _lib.NpdError(why)
        dev = next(self.parameters()).device
        y = _lib.f32c(_lib.stage(noisy_enc.detach(), "noisy_enc", dev))
        if y.dim() != 2 or y.shape[1] != self.output_len:
            raise ValueError(f"noisy_enc must be (batch, {self.output_len}), got {tuple(y.shape)}")
        if y.data_ptr() % 16:
            y = y.clone()
        B, p = y.shape[0], float(self.dropout.p)
        if drop_mult is not None:
            drop_mult = _lib.f32c(_lib.stage(drop_mult.detach(), "drop_mult", dev))
            if drop_mult.shape != y.shape:
                raise ValueError(f"drop_mult must be {tuple(y.shape)}, got {tuple(drop_mult.shape)}")
        elif p > 0.0:
            if p >= 1.0:
                drop_mult = torch.zeros_like(y)
            else:
                drop_mult = torch.bernoulli(torch.full_like(y, 1.0 - p)) / (1.0 - p)
        if B == 0:
            lg = torch.zeros(0, self.output_len, device=dev) + 0.0 * sum(q.sum() for q in self.parameters())
            return (lg, torch.zeros(0, self.hidden_dim // 2, self.output_len, device=dev)) if want_input4 else lg
        params, present = [], []
        for c in self._convs():
            params.append(c.weight)
            present.append(True)
            if c.bias is None:  # dont_use_bias: zeros in the flat vector, no gradient back
                params.append(torch.zeros(c.out_channels, dtype=torch.float32, device=dev))
                present.append(False)
            else:
                params.append(c.bias)
                present.append(True)
        for li in (0, 2, 4):
            params += [self.layersFin[li].weight, self.layersFin[li].bias]
        params += [self.layer_norm.weight, self.layer_norm.bias]
        present += [True] * 8
        plan = _conv_train_plan(dev, self.output_len, self.hidden_dim)
        lg, in4 = _ConvTrainFn.apply(plan, y, drop_mult, tuple(present), want_input4, *params)
        return (lg, in4) if want_input4 else lg

    def forward(self, noisy_enc, mask, trg_seq, device):
        """models.py:742-767: returns (output, decoded_msg_bits, out_mask, logits, input4), input4 being the
        (B, embed/2, N) activation after layers3 + residual, written out by the fused forward on request.

        In training mode logits (B, N, 1) carries the fused training kernels' grad_fn (train_logits: weights read from
        the device on every call, dropout drawn in Python), output and decoded_msg_bits are derived from it by torch
        ops, and input4 is DETACHED: a copy of the activation the forward kept for its backward, with no gradient (the
        reference's active losses never use it)."""
        if self.training:
            lg, in4 = self.train_logits(noisy_enc, want_input4=True)
            logits = _lib.home(lg, noisy_enc).unsqueeze(-1)
            out = torch.sigmoid(logits)
            return torch.cat((1 - out, out), -1), logits.detach().sign(), mask, logits, _lib.home(in4, noisy_enc)
        lg, dec, in4 = self.logits(noisy_enc, want_input4=True)
        logits = lg.unsqueeze(-1)
        out = torch.sigmoid(logits)
        return torch.cat((1 - out, out), -1), dec.unsqueeze(-1), mask, logits, in4

    def decode(self, noisy_enc, info_positions, mask, device, trg_seq=None):
        """models.py:769-772: (decoded_msg_bits (B,N,1), mask)."""
        _, dec = self.logits(noisy_enc)
        return dec.unsqueeze(-1), mask


class _ConvTrainPlan:
    """npd_conv_train handle of one (N, embed): the kernels' device image buffers, no weights."""

    def __init__(self, N, embed):
        out = ctypes.c_void_p()
        _lib.check(_lib.load().npd_conv_train_create(int(N), int(embed), ctypes.byref(out)), "npd_conv_train_create")
        self.h = out

    def workspace(self, B):
        sv, sc = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(_lib.load().npd_conv_train_workspace(self.h, int(B), ctypes.byref(sv), ctypes.byref(sc)),
                   "npd_conv_train_workspace")
        return sv.value, sc.value

    def __del__(self):
        try:
            if self.h:
                _lib.load().npd_conv_train_destroy(self.h)
        except Exception:
            pass


_CONV_TRAIN_PLANS = {}


def _conv_train_plan(device, N, embed):
    """One plan per (device, N, embed); the weights are passed per call, so nothing is keyed on them."""
    key = (str(device), int(N), int(embed))
    plan = _CONV_TRAIN_PLANS.get(key)
    if plan is None:
        with torch.cuda.device(device):
            plan = _CONV_TRAIN_PLANS[key] = _ConvTrainPlan(N, embed)
    return plan


class _ConvTrainFn(torch.autograd.Function):
    """(logits, input4) = npd_conv_train_forward(flat weights, y, drop_mult); backward = npd_conv_train_backward:
    per-parameter views of the flat gradient.

    The parameters (and y) are kept with ctx.save_for_backward: the backward packs its transposed images from the
    weights of the forward, so an in-place change of a parameter between forward and backward (an optimiser step
    before .backward()) raises through torch's version counter instead of mixing two sets of weights.  The plan's
    images are rewritten by every call, which is why the backward packs its own: two forwards may precede one backward
    on a shared plan."""

    @staticmethod
    def forward(ctx, plan, y, drop, present, want_input4, *params):
        dev = y.device
        B, N = y.shape
        flat = torch.cat([p.detach().reshape(-1) for p in params]).to(torch.float32).contiguous()
        n_saved, n_scratch = plan.workspace(B)
        saved = torch.empty(n_saved, dtype=torch.float32, device=dev)
        lg = torch.empty(B, N, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().npd_conv_train_forward(plan.h, _lib.ptr(flat), _lib.ptr(y), _lib.ptr(drop), _lib.ptr(lg),
                                                          _lib.ptr(saved), B, _lib.stream_of(dev)),
                       "npd_conv_train_forward")
        ctx.save_for_backward(y, *params)
        ctx.plan, ctx.saved_ws, ctx.n_scratch, ctx.drop, ctx.present = plan, saved, n_scratch, drop, present
        # include/npd.h: `saved` starts with z and the output of each conv layer; layer 5's output is input4
        H = params[0].shape[0]
        in4 = saved[11 * B * N * H:12 * B * N * H].view(B, N, H).permute(0, 2, 1).contiguous() if want_input4 \
            else torch.empty(0, device=dev)
        ctx.mark_non_differentiable(in4)
        return lg, in4

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout, _gin4):
        y, *params = ctx.saved_tensors  # raises if a parameter was changed in place since the forward
        plan, dev = ctx.plan, y.device
        flat = torch.cat([p.detach().reshape(-1) for p in params]).to(torch.float32).contiguous()
        g = gout.to(torch.float32).contiguous()
        scratch = torch.empty(ctx.n_scratch, dtype=torch.float32, device=dev)
        gflat = torch.empty_like(flat)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().npd_conv_train_backward(plan.h, _lib.ptr(flat), _lib.ptr(y), _lib.ptr(ctx.drop),
                                                           _lib.ptr(g), _lib.ptr(ctx.saved_ws), _lib.ptr(scratch),
                                                           _lib.ptr(gflat), y.shape[0], _lib.stream_of(dev)),
                       "npd_conv_train_backward")
        grads, off = [], 0
        for p, has in zip(params, ctx.present):
            n = p.numel()
            grads.append(gflat[off:off + n].view(p.shape) if has else None)
            off += n
        return (None, None, None, None, None) + tuple(grads)


# ------------------------------------------------------------------------------------ GPT transformer
def _sinusoid_table(n_position: int, d_hid: int, num: float = 10000.0) -> torch.Tensor:
    """(1, n_position, d_hid) fp32: sin at even, cos at odd features of pos / num^(2 (j // 2) / d_hid), from float64."""
    pos = np.arange(n_position, dtype=np.float64)[:, None]
    j = np.arange(d_hid)
    ang = pos / np.power(num, 2 * (j // 2) / d_hid)[None, :]
    ang[:, 0::2] = np.sin(ang[:, 0::2])
    ang[:, 1::2] = np.cos(ang[:, 1::2])
    return torch.FloatTensor(ang).unsqueeze(0)


class ScalarMult(nn.Module):
    """A learnt scalar the reference declares and never applies (kept so that its state dicts load strictly)."""

    def __init__(self):
        super().__init__()
        self.alpha = nn.Parameter(1e-10 * torch.ones(1))

    def forward(self, x):
        return self.alpha * x


class ScaledDotProductAttention(nn.Module):
    def __init__(self, temperature, attn_dropout=0.1):
        super().__init__()
        self.temperature = temperature
        self.dropout = nn.Dropout(attn_dropout)

    def forward(self, q, k, v, mask=None):
        attn = torch.matmul(q / self.temperature, k.transpose(2, 3))
        if mask is not None:
            attn = attn.masked_fill(mask == 0, -1e9)
        attn = self.dropout(torch.softmax(attn, dim=-1))
        return torch.matmul(attn, v), attn


class MultiHeadAttention(nn.Module):
    """Post-LN self-attention block: bias-free projections, residual, LayerNorm(eps 1e-6)."""

    def __init__(self, n_head, d_model, d_k, d_v, dropout=0.1):
        super().__init__()
        self.n_head, self.d_k, self.d_v = n_head, d_k, d_v
        self.w_qs = nn.Linear(d_model, n_head * d_k, bias=False)
        self.w_ks = nn.Linear(d_model, n_head * d_k, bias=False)
        self.w_vs = nn.Linear(d_model, n_head * d_v, bias=False)
        self.fc = nn.Linear(n_head * d_v, d_model, bias=False)
        self.attention = ScaledDotProductAttention(temperature=d_k ** 0.5)
        self.dropout = nn.Dropout(dropout)
        self.layer_norm = nn.LayerNorm(d_model, eps=1e-6)
        self.scalar = ScalarMult()

    def forward(self, q, k, v, mask=None):
        B, lq, lk = q.size(0), q.size(1), k.size(1)
        residual = q
        q = self.w_qs(q).view(B, lq, self.n_head, self.d_k).transpose(1, 2)
        k = self.w_ks(k).view(B, lk, self.n_head, self.d_k).transpose(1, 2)
        v = self.w_vs(v).view(B, lk, self.n_head, self.d_v).transpose(1, 2)
        if mask is not None:
            mask = mask.unsqueeze(1)
        o, attn = self.attention(q, k, v, mask=mask)
        o = self.dropout(self.fc(o.transpose(1, 2).contiguous().view(B, lq, -1)))
        return self.layer_norm(o + residual), attn


class PositionwiseFeedForward(nn.Module):
    def __init__(self, d_in, d_hid, dropout=0.1):
        super().__init__()
        self.w_1 = nn.Linear(d_in, d_hid)
        self.w_2 = nn.Linear(d_hid, d_in)
        self.layer_norm = nn.LayerNorm(d_in, eps=1e-6)
        self.dropout = nn.Dropout(dropout)
        self.scalar = ScalarMult()

    def forward(self, x):
        return self.layer_norm(self.dropout(self.w_2(torch.nn.functional.gelu(self.w_1(x)))) + x)


class EncoderLayer(nn.Module):
    def __init__(self, d_model, d_inner, n_head, d_k, d_v, dropout=0.1):
        super().__init__()
        self.slf_attn = MultiHeadAttention(n_head, d_model, d_k, d_v, dropout=dropout)
        self.pos_ffn = PositionwiseFeedForward(d_model, d_inner, dropout=dropout)

    def forward(self, x, slf_attn_mask=None):
        x, attn = self.slf_attn(x, x, x, mask=slf_attn_mask)
        return self.pos_ffn(x), attn


class PositionalEncoding(nn.Module):
    def __init__(self, d_hid, n_position=200, num=10000):
        super().__init__()
        self.register_buffer("pos_table", _sinusoid_table(n_position, d_hid, num))

    def forward(self, x):
        return x + self.pos_table[:, :x.size(1)].clone().detach()


class XFormerGPT(nn.Module):
    """The layer stack (models.py:299-336); layer_norm and layer_norm_cross exist and are never applied."""

    def __init__(self, config):
        super().__init__()
        self.embed_dim = config.embed_dim
        self.block_len = config.max_len
        self.position_enc_auto = PositionalEncoding(self.embed_dim, n_position=self.block_len)
        self.dropout = nn.Dropout(p=config.dropout)
        d = config.embed_dim // config.n_head
        self.layer_stack = nn.ModuleList([EncoderLayer(config.embed_dim, config.embed_dim * 4, config.n_head, d, d,
                                                       dropout=config.dropout) for _ in range(config.n_layers)])
        self.layer_norm = nn.LayerNorm(config.embed_dim, eps=1e-6)
        self.layer_norm_cross = nn.LayerNorm(config.embed_dim, eps=1e-6)

    def forward(self, trg_seq, trg_mask, device=None):
        x = self.dropout(self.position_enc_auto(trg_seq))
        for layer in self.layer_stack:
            x, _ = layer(x, slf_attn_mask=trg_mask)
        return x


class XFormerEndToEndGPT(nn.Module):
    """Drop-in for models.XFormerEndToEndGPT (models.py:340-423), the reference's default ``--model gpt``.

    ``decode`` / ``decode_logits`` run the whole successive decode in one launch of libnpd's fused kernel
    (npd_gpt_decode): at every information position the layer stack runs on the prefix built so far, every token
    attending to every key up to that position.  ``forward`` (teacher-forced, causal; the training-time API) is plain
    torch.  The kernel covers embed_dim 64, n_head 8, N = max_len in {16, 32, 64}, 1 .. 8 layers
    (:meth:`fused_supported`); anything else raises NpdError -- there is no eager fall-back."""

    def __init__(self, config):
        super().__init__()
        self.embed_dim = config.embed_dim
        self.block_len = config.max_len
        self.N = config.N
        self.n_head = config.n_head
        self.n_layers = config.n_layers
        self.trg_pad_idx = 2
        e = self.embed_dim
        self.start_embed_layer = nn.Sequential(nn.Linear(config.N, e), nn.GELU(), nn.Linear(e, e), nn.GELU(),
                                               nn.Linear(e, e))
        self.learnt_pos = True
        self.pos_emb = nn.Embedding(self.block_len, e)
        self.layer_norm_inp = nn.LayerNorm(e, eps=1e-6)
        self.layer_norm_out = nn.LayerNorm(e, eps=1e-6)
        self.Decoder = XFormerGPT(config)
        self.Lin_Decoder = nn.Linear(e, 1)
        self._handle = None
        self._hkey = None

    # ------------------------------------------------------------------ teacher-forced forward (plain torch)
    def forward(self, noisy_enc, mask, trg_seq, device):
        """models.py:365-396: (output (B,N,2), decoded_msg_bits (B,N,1), mask, logits (B,N,1)); token j is built from
        trg_seq[:, j-1], attention is causal."""
        B = trg_seq.size(0)
        seq = torch.cat((torch.ones((B, 1), device=device), trg_seq[:, :-1]), -1)
        L = seq.size(1)
        causal = torch.tril(torch.ones((1, L, L), device=device)).bool()
        trg_mask = (seq != self.trg_pad_idx).unsqueeze(-2) & causal
        tok = seq.unsqueeze(-1) * self.pos_emb(torch.arange(self.block_len, device=device))
        tok = torch.cat((self.start_embed_layer(noisy_enc).unsqueeze(1), tok[:, 1:]), 1)
        logits = self.Lin_Decoder(self.Decoder(tok, trg_mask, device))
        out = torch.sigmoid(logits)
        return torch.cat((1 - out, out), -1), logits.sign(), mask, logits

    # ------------------------------------------------------------------ fused path
    def fused_reason(self) -> str:
        """Why the fused kernel does not cover this configuration ('' if it does)."""
        if self.embed_dim != 64:
            return f"embed_dim {self.embed_dim}: the fused GPT kernel is built for embed_dim 64"
        if self.n_head != 8:
            return f"n_head {self.n_head}: the fused GPT kernel is built for 8 heads"
        if self.block_len != self.N:
            return f"max_len {self.block_len} != N {self.N}: the fused GPT kernel needs max_len == N"
        if self.N not in (16, 32, 64):
            return f"N {self.N}: the fused GPT kernel covers N in (16, 32, 64)"
        if not 1 <= self.n_layers <= 8:
            return f"n_layers {self.n_layers}: the fused GPT kernel covers 1 .. 8 layers"
        return ""

    def fused_supported(self) -> bool:
        return self.fused_reason() == ""

    def _packed(self) -> np.ndarray:
        """The weights npd_gpt_create reads, in the order include/npd.h documents."""
        def a(t):
            return t.detach().float().cpu().numpy().ravel()
        parts = []
        for li in (0, 2, 4):
            parts += [a(self.start_embed_layer[li].weight), a(self.start_embed_layer[li].bias)]
        parts += [a(self.pos_emb.weight), a(self.Decoder.position_enc_auto.pos_table[0, :self.N])]
        for layer in self.Decoder.layer_stack:
            at, ff = layer.slf_attn, layer.pos_ffn
            parts += [a(at.w_qs.weight), a(at.w_ks.weight), a(at.w_vs.weight), a(at.fc.weight),
                      a(at.layer_norm.weight), a(at.layer_norm.bias), a(ff.w_1.weight), a(ff.w_1.bias),
                      a(ff.w_2.weight), a(ff.w_2.bias), a(ff.layer_norm.weight), a(ff.layer_norm.bias)]
        parts += [a(self.Lin_Decoder.weight), a(self.Lin_Decoder.bias)]
        return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)

    def _get_handle(self, device):
        tensors = list(self.parameters()) + [self.Decoder.position_enc_auto.pos_table]
        key = (str(device), tuple(p._version for p in tensors), tuple(p.data_ptr() for p in tensors))
        if self._handle is None or self._hkey != key:
            W = self._packed()
            out = ctypes.c_void_p()
            L = _lib.load()
            with torch.cuda.device(device):
                _lib.check(L.npd_gpt_create(int(self.N), int(self.embed_dim), int(self.n_head), int(self.n_layers),
                                            W.ctypes.data_as(ctypes.c_void_p), int(W.size), ctypes.byref(out)),
                           "npd_gpt_create")
            if self._handle is not None:
                L.npd_gpt_destroy(self._handle)
            self._handle, self._hkey = out, key
        return self._handle

    def __del__(self):
        try:
            if self._handle is not None:
                _lib.load().npd_gpt_destroy(self._handle)
        except Exception:
            pass

    def _is_info(self, info_positions) -> np.ndarray:
        info = np.asarray(info_positions.cpu() if isinstance(info_positions, torch.Tensor) else info_positions)
        info = info.astype(np.int64).ravel()
        if info.size and (info.min() < 0 or info.max() >= self.N):
            raise ValueError("info_positions must lie in 0 .. N - 1")
        m = np.zeros(self.N, dtype=np.uint8)
        m[info] = 1
        return m

    def decode_logits(self, y, info_positions, forced=None):
        """(bits (B,N), logits (B,N)) of the successive decode; logits are 0 and bits +1 at frozen positions.  With
        ``forced`` (B,N) of +-1, token j is built from forced[:, j-1] instead of the decision (the bits returned are
        still the signs of the logits)."""
        reason = self.fused_reason()
        if reason:
            raise _lib.NpdError(reason)
        if self.training:
            raise _lib.NpdError("the fused GPT path is inference-only (eval mode)")
        if y.dim() != 2 or y.shape[1] != self.N:
            raise ValueError("input must be (B, N) with N = config.N")
        is_info = self._is_info(info_positions)
        yd = _lib.f32c(_lib.stage(y, "noisy_enc"))
        B = yd.shape[0]
        fd = None
        if forced is not None:
            if tuple(forced.shape) != (B, self.N):
                raise ValueError("forced must be (B, N)")
            fd = _lib.f32c(_lib.stage(forced, "forced", yd.device))
        h = self._get_handle(yd.device)
        bits = torch.empty(B, self.N, dtype=torch.float32, device=yd.device)
        lg = torch.empty_like(bits)
        L = _lib.load()
        with torch.cuda.device(yd.device):
            _lib.check(L.npd_gpt_decode(h, _lib.ptr(yd), is_info.ctypes.data_as(ctypes.c_void_p), _lib.ptr(fd),
                                        _lib.ptr(bits), _lib.ptr(lg), B, _lib.stream_of(yd.device)), "npd_gpt_decode")
        return _lib.home(bits, y), _lib.home(lg, y)

    def decode(self, noisy_enc, info_positions, mask, device):
        """models.py:398-423: (output_bits (B,N), mask).  Every test-time caller passes an all-ones mask
        (run_models.py:326); anything else is refused."""
        if mask is not None and not bool(torch.as_tensor(mask).all()):
            raise _lib.NpdError("the fused GPT decode takes an all-ones mask (run_models.py:326)")
        bits, _ = self.decode_logits(noisy_enc, info_positions)
        return bits, mask


# ------------------------------------------------------------------- encoder / decoder transformer models
class DecoderLayer(nn.Module):
    """Self-attention, cross-attention over the memory, FFN (models.py:178-197)."""

    def __init__(self, d_model, d_inner, n_head, d_k, d_v, dropout=0.1):
        super().__init__()
        self.slf_attn = MultiHeadAttention(n_head, d_model, d_k, d_v, dropout=dropout)
        self.enc_attn = MultiHeadAttention(n_head, d_model, d_k, d_v, dropout=dropout)
        self.pos_ffn = PositionwiseFeedForward(d_model, d_inner, dropout=dropout)

    def forward(self, x, mem, slf_attn_mask=None, dec_enc_attn_mask=None):
        x, slf = self.slf_attn(x, x, x, mask=slf_attn_mask)
        x, cross = self.enc_attn(x, mem, mem, mask=dec_enc_attn_mask)
        return self.pos_ffn(x), slf, cross


def _key_mask(mask):
    """A (b, L) mask over the keys of each word, in the (b, 1, L) form MultiHeadAttention broadcasts over heads and
    queries -- the reference's masking branch for these two models."""
    return None if mask is None else mask.unsqueeze(1)


class XFormerEncoder(nn.Module):
    """models.py:223-250: token j = LayerNorm(y_j pos_emb[j+1] + table[j]), then the encoder layers."""

    def __init__(self, config):
        super().__init__()
        self.embed_dim = config.embed_dim
        self.block_len = config.max_len
        self.pos_emb = nn.Embedding(config.N + 1, config.embed_dim, padding_idx=0)
        self.position_enc = PositionalEncoding(self.embed_dim, n_position=self.block_len)
        self.dropout = nn.Dropout(p=config.dropout)
        d = config.embed_dim // config.n_head
        self.layer_stack = nn.ModuleList([EncoderLayer(config.embed_dim, config.embed_dim * 4, config.n_head, d, d,
                                                       dropout=config.dropout) for _ in range(config.n_layers)])
        self.layer_norm = nn.LayerNorm(config.embed_dim, eps=1e-6)

    def forward(self, noisy_enc, src_mask, device):
        """noisy_enc (b, L, E): y repeated over the features; src_mask (b, L) over the keys."""
        x = noisy_enc * self.pos_emb(torch.arange(1, self.block_len + 1, device=device))
        x = self.layer_norm(self.dropout(self.position_enc(x)))
        for layer in self.layer_stack:
            x, _ = layer(x, slf_attn_mask=_key_mask(src_mask))
        return x


class XFormerDecoder(nn.Module):
    """models.py:252-297: the memory is LayerNorm_cross(y_j emb_cross[j+1] + table_5000[j]) (no encoder stack), the
    tokens LayerNorm(emb_inputs[idx_t] + table_10000[t]); every layer cross-attends.  emb_auto is never read."""

    def __init__(self, config):
        super().__init__()
        self.embed_dim = config.embed_dim
        self.block_len = config.max_len
        self.emb_auto = nn.Embedding(config.N + 1, config.embed_dim, padding_idx=0)
        self.emb_cross = nn.Embedding(config.N + 1, config.embed_dim, padding_idx=0)
        self.emb_inputs = nn.Embedding(4, config.embed_dim, padding_idx=3)
        self.position_enc_auto = PositionalEncoding(self.embed_dim, n_position=self.block_len)
        self.position_enc_cross = PositionalEncoding(self.embed_dim, n_position=self.block_len, num=5000)
        self.dropout = nn.Dropout(p=config.dropout)
        self.dropout_cross = nn.Dropout(p=config.dropout)
        d = config.embed_dim // config.n_head
        self.layer_stack = nn.ModuleList([DecoderLayer(config.embed_dim, config.embed_dim * 4, config.n_head, d, d,
                                                       dropout=config.dropout) for _ in range(config.n_layers)])
        self.layer_norm = nn.LayerNorm(config.embed_dim, eps=1e-6)
        self.layer_norm_cross = nn.LayerNorm(config.embed_dim, eps=1e-6)

    def forward(self, noisy_enc, src_mask, trg_seq, trg_mask, device):
        """noisy_enc (b, L, E); trg_seq (b, L) of token indices; src_mask, trg_mask (b, L) over the keys."""
        mem = noisy_enc * self.emb_cross(torch.arange(1, self.block_len + 1, device=device))
        mem = self.layer_norm_cross(self.dropout_cross(self.position_enc_cross(mem)))
        x = self.layer_norm(self.dropout(self.position_enc_auto(self.emb_inputs(trg_seq))))
        for layer in self.layer_stack:
            x, _, _ = layer(x, mem, slf_attn_mask=_key_mask(trg_mask), dec_enc_attn_mask=_key_mask(src_mask))
        return x


class _FusedXFormer(nn.Module):
    """What the two classes below share: the coverage of their fused kernels, the refusals and the handle cache."""

    _prefix = ""   # C entry points: <prefix>_create / _destroy
    _label = ""

    def _init_common(self, config):
        self.embed_dim = config.embed_dim
        self.block_len = config.max_len
        self.N = config.N
        self.n_head = config.n_head
        self.n_layers = config.n_layers
        self._handle = None
        self._hkey = None

    def fused_reason(self) -> str:
        """Why the fused kernel does not cover this configuration ('' if it does)."""
        k = f"the fused {self._label} kernel"
        if self.embed_dim != 64:
            return f"embed_dim {self.embed_dim}: {k} is built for embed_dim 64"
        if self.n_head != 8:
            return f"n_head {self.n_head}: {k} is built for 8 heads"
        if self.block_len != self.N:
            return f"max_len {self.block_len} != N {self.N}: {k} needs max_len == N"
        if self.N not in (16, 32, 64):
            return f"N {self.N}: {k} covers N in (16, 32, 64)"
        if not 1 <= self.n_layers <= 8:
            return f"n_layers {self.n_layers}: {k} covers 1 .. 8 layers"
        return ""

    def fused_supported(self) -> bool:
        return self.fused_reason() == ""

    def _get_handle(self, device):
        tensors = list(self.parameters()) + list(self.buffers())
        key = (str(device), tuple(p._version for p in tensors), tuple(p.data_ptr() for p in tensors))
        if self._handle is None or self._hkey != key:
            W = self._packed()
            out = ctypes.c_void_p()
            L = _lib.load()
            with torch.cuda.device(device):
                _lib.check(getattr(L, self._prefix + "_create")(int(self.N), int(self.embed_dim), int(self.n_head),
                                                                int(self.n_layers), W.ctypes.data_as(ctypes.c_void_p),
                                                                int(W.size), ctypes.byref(out)),
                           self._prefix + "_create")
            if self._handle is not None:
                getattr(L, self._prefix + "_destroy")(self._handle)
            self._handle, self._hkey = out, key
        return self._handle

    def __del__(self):
        try:
            if self._handle is not None:
                getattr(_lib.load(), self._prefix + "_destroy")(self._handle)
        except Exception:
            pass

    def _check_mask(self, mask):
        """Every test-time caller passes an all-ones mask (run_models.py:326); anything else is refused."""
        if mask is not None and not bool(torch.as_tensor(mask).all()):
            raise _lib.NpdError(f"the fused {self._label} path takes an all-ones mask (run_models.py:326)")

    def _check(self, y):
        """The refusals every fused call makes, before anything moves to the device."""
        reason = self.fused_reason()
        if reason:
            raise _lib.NpdError(reason)
        if self.training:
            raise _lib.NpdError(f"the fused {self._label} path is inference-only (eval mode)")
        if y.dim() != 2 or y.shape[1] != self.N:
            raise ValueError("input must be (B, N) with N = config.N")

    @staticmethod
    def _layer_parts(a, at, ff=None):
        parts = [a(at.w_qs.weight), a(at.w_ks.weight), a(at.w_vs.weight), a(at.fc.weight), a(at.layer_norm.weight),
                 a(at.layer_norm.bias)]
        if ff is not None:
            parts += [a(ff.w_1.weight), a(ff.w_1.bias), a(ff.w_2.weight), a(ff.w_2.bias), a(ff.layer_norm.weight),
                      a(ff.layer_norm.bias)]
        return parts


def _flat(t):
    return t.detach().float().cpu().numpy().ravel()


class XFormerEndToEndEncoder(_FusedXFormer):
    """Drop-in for models.XFormerEndToEndEncoder (models.py:662-686, ``--model encoder``): one pass over the N tokens,
    a logit for each.  ``decode`` / ``logits`` run in one launch of libnpd's fused kernel (npd_xfenc_forward);
    ``forward`` (the training-time API, any mask) is plain torch.  The kernel covers embed_dim 64, n_head 8,
    N = max_len in {16, 32, 64}, 1 .. 8 layers; anything else raises NpdError -- there is no eager fall-back."""

    _prefix, _label = "npd_xfenc", "encoder"

    def __init__(self, config):
        super().__init__()
        self._init_common(config)
        self.Encoder = XFormerEncoder(config)
        self.Lin_Decoder = nn.Linear(config.embed_dim, 1)

    def forward(self, noisy_enc, mask, trg_seq, device):
        """models.py:671-681: (output (B,N,2), decoded_msg_bits (B,N,1), mask, logits (B,N,1))."""
        x = torch.ones(self.embed_dim, device=device) * noisy_enc.unsqueeze(-1)
        logits = self.Lin_Decoder(self.Encoder(x, mask, device))
        out = torch.sigmoid(logits)
        return torch.cat((1 - out, out), -1), logits.sign(), mask, logits

    def _packed(self) -> np.ndarray:
        """The weights npd_xfenc_create reads, in the order include/npd.h documents."""
        a, enc = _flat, self.Encoder
        parts = [a(enc.pos_emb.weight), a(enc.position_enc.pos_table[0, :self.N]), a(enc.layer_norm.weight),
                 a(enc.layer_norm.bias)]
        for layer in enc.layer_stack:
            parts += self._layer_parts(a, layer.slf_attn, layer.pos_ffn)
        parts += [a(self.Lin_Decoder.weight), a(self.Lin_Decoder.bias)]
        return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)

    def logits(self, y):
        """(logits (B,N), bits (B,N)): the sign is taken at every position, frozen ones included."""
        self._check(y)
        yd = _lib.f32c(_lib.stage(y, "noisy_enc"))
        B = yd.shape[0]
        h = self._get_handle(yd.device)
        bits = torch.empty(B, self.N, dtype=torch.float32, device=yd.device)
        lg = torch.empty_like(bits)
        with torch.cuda.device(yd.device):
            _lib.check(_lib.load().npd_xfenc_forward(h, _lib.ptr(yd), _lib.ptr(bits), _lib.ptr(lg), B,
                                                     _lib.stream_of(yd.device)), "npd_xfenc_forward")
        return _lib.home(lg, y), _lib.home(bits, y)

    def decode(self, noisy_enc, info_positions, mask, device, trg_seq=None):
        """models.py:683-686: (decoded_msg_bits (B,N,1), mask); an all-ones mask only."""
        self._check_mask(mask)
        _, bits = self.logits(noisy_enc)
        return bits.unsqueeze(-1), mask


class XFormerEndToEndDecoder(_FusedXFormer):
    """Drop-in for models.XFormerEndToEndDecoder (models.py:599-654, ``--model decoder``): autoregressive, with
    cross-attention over an embedding of y in every layer.  ``decode`` / ``decode_logits`` run the whole successive
    decode in one launch of libnpd's fused kernel (npd_xfdec_decode); ``forward`` (teacher-forced, each word expanded
    to max_len rows; the training-time API) is plain torch.  Coverage and refusals as for the encoder."""

    _prefix, _label = "npd_xfdec", "decoder"

    def __init__(self, config):
        super().__init__()
        self._init_common(config)
        self.trg_pad_idx = 3
        self.start_idx = 2
        self.Decoder = XFormerDecoder(config)
        self.Lin_Decoder = nn.Linear(config.embed_dim, 1)

    def forward(self, noisy_enc, mask, trg_seq, device):
        """models.py:609-633.  Word b becomes max_len rows; row b max_len + t holds the tokens built from
        trg_seq[b, :-1] behind the start token, with the keys <= t, so its logit at position t is the decode's at step
        t along that path.  Returns (output (B L, L, 2), decoded_msg_bits (B L, L, 1), out_mask (B L, L) -- one at
        position t of row b L + t --, logits (B L, L, 1))."""
        B = trg_seq.size(0)
        idx = torch.cat((torch.full((B, 1), self.start_idx, dtype=torch.long, device=device),
                         (trg_seq[:, :-1] == 1).long()), -1)
        L = idx.size(1)
        causal = torch.tril(torch.ones((1, L, L), device=device)).bool()
        trg_mask = ((idx != self.trg_pad_idx).unsqueeze(-2) & causal).reshape(B * L, L)
        shifted = torch.cat((trg_mask[:, 1:].float(), torch.zeros((B * L, 1), device=device)), -1)
        idx = idx.repeat_interleave(L, 0)
        y = noisy_enc.repeat_interleave(L, 0)
        src_mask = torch.as_tensor(mask, device=device).repeat_interleave(L, 0)
        x = torch.ones(self.embed_dim, device=device) * y.unsqueeze(-1)
        logits = self.Lin_Decoder(self.Decoder(x, src_mask, idx, trg_mask, device))
        out = torch.sigmoid(logits)
        return torch.cat((1 - out, out), -1), logits.sign(), trg_mask.float() - shifted, logits

    def _packed(self) -> np.ndarray:
        """The weights npd_xfdec_create reads, in the order include/npd.h documents."""
        a, dec = _flat, self.Decoder
        parts = [a(dec.emb_cross.weight), a(dec.position_enc_cross.pos_table[0, :self.N]),
                 a(dec.layer_norm_cross.weight), a(dec.layer_norm_cross.bias), a(dec.emb_inputs.weight),
                 a(dec.position_enc_auto.pos_table[0, :self.N]), a(dec.layer_norm.weight), a(dec.layer_norm.bias)]
        for layer in dec.layer_stack:
            parts += self._layer_parts(a, layer.slf_attn) + self._layer_parts(a, layer.enc_attn, layer.pos_ffn)
        parts += [a(self.Lin_Decoder.weight), a(self.Lin_Decoder.bias)]
        return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)

    _is_info = XFormerEndToEndGPT._is_info

    def decode_logits(self, y, info_positions, forced=None):
        """(bits (B,N), logits (B,N)) of the successive decode; logits are 0 and bits +1 at frozen positions.  With
        ``forced`` (B,N) of +-1, token j is built from forced[:, j-1] instead of the decision (the bits returned are
        still the signs of the logits)."""
        self._check(y)
        is_info = self._is_info(info_positions)
        if forced is not None and tuple(forced.shape) != tuple(y.shape):
            raise ValueError("forced must be (B, N)")
        yd = _lib.f32c(_lib.stage(y, "noisy_enc"))
        B = yd.shape[0]
        fd = None if forced is None else _lib.f32c(_lib.stage(forced, "forced", yd.device))
        h = self._get_handle(yd.device)
        bits = torch.empty(B, self.N, dtype=torch.float32, device=yd.device)
        lg = torch.empty_like(bits)
        with torch.cuda.device(yd.device):
            _lib.check(_lib.load().npd_xfdec_decode(h, _lib.ptr(yd), is_info.ctypes.data_as(ctypes.c_void_p),
                                                    _lib.ptr(fd), _lib.ptr(bits), _lib.ptr(lg), B,
                                                    _lib.stream_of(yd.device)), "npd_xfdec_decode")
        return _lib.home(bits, y), _lib.home(lg, y)

    def decode(self, noisy_enc, info_positions, mask, device):
        """models.py:635-654: (output_bits (B,N), mask); an all-ones mask only."""
        self._check_mask(mask)
        bits, _ = self.decode_logits(noisy_enc, info_positions)
        return bits, mask
