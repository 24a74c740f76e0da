"""The "transpeaker" — the transformer speaker of the fine-tuning loop's back-translation augmentation (last item):
`Transpeaker` of M/models/transpeaker_model.py:232-257 (M = /root/reference/map_nav_src) on the HIP kernels, with the reference's
`state_dict` keys, plus the two uses of it in M/r2r/transpeaker.py: the teacher-forced loss (:209-246) and greedy / sampled decoding
(`infer_batch`, :248-318), and the feature walk along the ground-truth path (`from_shortest_path`, :158-199) on navsim.GraphSim.

Reference behaviour kept (file:line in M/models/transpeaker_model.py):
  * MultiHeadAttention (:91-119): bias-free projections, heads of size `aemb` (64: the head size of goat_attn_*), boolean masks filled
    with -1e9 BEFORE the softmax (a fully masked row becomes uniform, not NaN), `LayerNorm(out + residual)` with a LayerNorm built
    inside forward — never trained: unit gain, zero shift, eps 1e-5 — then dropout;
  * the attention-probability dropout lives in a module created inside forward (:98,114) and is therefore ACTIVE IN EVAL MODE too
    (p = speaker_dropout); reproduced: `attn_dropout_always`.  Q / K / V dropout only with `use_drop` (:110-113);
  * PositionalEncoding (:32-48): sinusoid table added over the sequence axis, dropout 0.1;
  * PoswiseFeedForwardNet (:121-134): Linear - ReLU - Dropout - Linear without biases, LayerNorm(out + x) as above;
  * encoder (:158-198): per step the action feature [F] attends over the 36 view features [36, F] (one query, no mask), the T step
    vectors then pass `speaker_layer_num` encoder layers WITHOUT a padding mask; decoder (:200-230): pad + causal self-attention
    mask, optional context mask, weight-tied to nothing (projection is its own Linear).
"""
import math

import numpy as np
import torch
from torch import nn

from . import hipops
from . import layers
from .layers import compute_dtype, _p


def _sinusoid(max_len, d_model):
    pe = torch.zeros(max_len, d_model)
    position = torch.arange(0, max_len, dtype=torch.float).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d_model, 2).float() * (-math.log(10000.0) / d_model))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe.unsqueeze(0).transpose(0, 1)          # [max_len, 1, d_model] (the reference's buffer shape: state_dict key `pe`)


class PositionalEncoding(nn.Module):
    def __init__(self, d_model, dropout=0.1, max_len=5000):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        self.register_buffer('pe', _sinusoid(max_len, d_model))

    def forward(self, x):
        """x [B, L, D] (batch first here; the reference transposes around the call)."""
        y = x + self.pe[:x.shape[1], 0].to(x.dtype).unsqueeze(0)
        return hipops.dropout(y, _p(self.dropout))


class _NoAffineLN(nn.Module):
    """nn.LayerNorm(hidden)(x) of a module built inside forward (never trained): gain 1, shift 0, eps 1e-5."""

    def __init__(self, hidden):
        super().__init__()
        self.register_buffer('one', torch.ones(hidden), persistent=False)
        self.register_buffer('zero', torch.zeros(hidden), persistent=False)

    def forward(self, x, residual, p=0.0):
        return hipops.layer_norm(x, self.one, self.zero, 1e-5, residual=residual)


class MultiHeadAttention(nn.Module):
    def __init__(self, q_hidden, k_hidden, n_heads, cfg):
        super().__init__()
        d_k = cfg.aemb
        if d_k != 64:
            raise NotImplementedError('GOAT HIP attention kernels are specialised for head size 64 (aemb)')
        self.n_heads, self.hidden = n_heads, q_hidden
        self.W_Q = nn.Linear(q_hidden, d_k * n_heads, bias=False)
        self.W_K = nn.Linear(k_hidden, d_k * n_heads, bias=False)
        self.W_V = nn.Linear(k_hidden, d_k * n_heads, bias=False)
        self.fc = nn.Linear(n_heads * d_k, q_hidden, bias=False)
        self.dropout = nn.Dropout(cfg.speaker_dropout)
        self.ln = _NoAffineLN(q_hidden)
        self.use_drop = bool(getattr(cfg, 'use_drop', False))
        self.attn_p = float(cfg.speaker_dropout) if getattr(cfg, 'attn_dropout_always', True) else None

    def forward(self, xq, xkv, bias=None):
        """xq [B, Lq, q_hidden], xkv [B, Lk, k_hidden]; bias: float32 [B, Lq, Lk] additive mask (0 / -1e9) or None."""
        q = hipops.linear(xq, self.W_Q.weight)
        k = hipops.linear(xkv, self.W_K.weight)
        v = hipops.linear(xkv, self.W_V.weight)
        if self.use_drop:
            q, k, v = (hipops.dropout(t, _p(self.dropout)) for t in (q, k, v))
        p = self.attn_p if self.attn_p is not None else _p(self.dropout)       # (the reference's always-on attention dropout)
        ctx = hipops.attention(q, torch.cat([k, v], -1), None, bias, self.n_heads, p)
        out = self.ln(hipops.linear(ctx, self.fc.weight), xq)
        return hipops.dropout(out, _p(self.dropout))


class PoswiseFeedForwardNet(nn.Module):
    def __init__(self, hidden, cfg):
        super().__init__()
        self.fc = nn.Sequential(nn.Linear(hidden, cfg.proj_hidden, bias=False), nn.ReLU(), nn.Dropout(cfg.speaker_dropout),
                                nn.Linear(cfg.proj_hidden, hidden, bias=False))
        self.ln = _NoAffineLN(hidden)

    def forward(self, x):
        h = hipops.linear(x, self.fc[0].weight, None, 'relu')
        h = hipops.dropout(h, _p(self.fc[2]))
        return self.ln(hipops.linear(h, self.fc[3].weight), x)


class EncoderLayer(nn.Module):
    def __init__(self, hidden, n_heads, cfg):
        super().__init__()
        self.enc_self_attn = MultiHeadAttention(hidden, hidden, n_heads, cfg)
        self.pos_ffn = PoswiseFeedForwardNet(hidden, cfg)

    def forward(self, x):
        return self.pos_ffn(self.enc_self_attn(x, x))


class DecoderLayer(nn.Module):
    def __init__(self, q_size, k_size, n_heads, cfg):
        super().__init__()
        self.dec_self_attn = MultiHeadAttention(q_size, q_size, n_heads, cfg)
        self.dec_enc_attn = MultiHeadAttention(q_size, k_size, n_heads, cfg)
        self.pos_ffn = PoswiseFeedForwardNet(q_size, cfg)

    def forward(self, x, enc, self_bias, enc_bias):
        x = self.dec_self_attn(x, x, self_bias)
        x = self.dec_enc_attn(x, enc, enc_bias)
        return self.pos_ffn(x)


class TranspeakerEncoder(nn.Module):
    def __init__(self, feature_size, hidden, cfg):
        super().__init__()
        self.hidden_size, self.feature_size, self.image_feat_size = hidden, feature_size, cfg.image_feat_size
        self.pos_emb = PositionalEncoding(hidden)
        self.drop_feat = nn.Dropout(p=cfg.featdropout)
        self.drop = nn.Dropout(p=cfg.speaker_dropout)
        self.down_size = nn.Linear(feature_size, hidden)
        self.layers = nn.ModuleList([EncoderLayer(hidden, cfg.speaker_head_num, cfg) for _ in range(cfg.speaker_layer_num)])
        self.image_self_attn = MultiHeadAttention(hidden, feature_size, cfg.speaker_head_num, cfg)

    def _drop_image_part(self, x):
        p = _p(self.drop_feat)
        if p <= 0:
            return x
        D = self.image_feat_size
        return torch.cat([hipops.dropout(x[..., :D].contiguous(), p), x[..., D:]], -1)

    def forward(self, action_inputs, feature_inputs, already_dropfeat=False):
        """action_inputs [B, T, F] (the view taken at each step + its angle feature), feature_inputs [B, T, 36, F]."""
        dt = compute_dtype()
        B, T, F = action_inputs.shape
        a, f = action_inputs.to(dt), feature_inputs.to(dt)
        if not already_dropfeat:
            a, f = self._drop_image_part(a), self._drop_image_part(f)
        ctx = hipops.linear(a, self.down_size.weight, self.down_size.bias).reshape(B * T, 1, self.hidden_size)
        enc_inputs = self.image_self_attn(ctx, f.reshape(B * T, 36, F)).view(B, T, self.hidden_size)
        x = self.pos_emb(enc_inputs)
        for layer in self.layers:
            x = layer(x)
        return enc_inputs, x


class TranspeakerDecoder(nn.Module):
    def __init__(self, vocab, word_size, hidden, padding_idx, cfg):
        super().__init__()
        self.embedding = nn.Embedding(vocab, word_size, padding_idx)
        self.pos_emb = PositionalEncoding(word_size)
        self.layers = nn.ModuleList([DecoderLayer(word_size, hidden, cfg.speaker_head_num, cfg) for _ in range(cfg.speaker_layer_num)])
        self.drop = nn.Dropout(p=cfg.speaker_dropout)
        self.use_drop = bool(getattr(cfg, 'use_drop', False))

    def forward(self, dec_inputs, enc_outputs, ctx_mask=None):
        """dec_inputs int64 [B, L]; ctx_mask bool [B, T] (True = padded context step) or None."""
        dt = compute_dtype()
        ids = dec_inputs.to(torch.int64)
        B, L = ids.shape
        x = hipops.embedding(ids, self.embedding.weight, out_dtype=dt, word_pad=self.embedding.padding_idx)
        if self.use_drop:
            x = hipops.dropout(x, _p(self.drop))
        x = self.pos_emb(x)
        # pad (key == 0) or future position -> -1e9 (:212-214)
        masked = ids.eq(0).unsqueeze(1) | torch.triu(torch.ones(L, L, dtype=torch.bool, device=ids.device), 1).unsqueeze(0)
        self_bias = torch.zeros(B, L, L, dtype=torch.float32, device=ids.device).masked_fill_(masked, -1e9)
        enc_bias = None
        if ctx_mask is not None:
            T = ctx_mask.shape[1]
            enc_bias = torch.zeros(B, L, T, dtype=torch.float32, device=ids.device).masked_fill_(ctx_mask.bool().unsqueeze(1), -1e9)
        enc = enc_outputs.to(dt)
        for layer in self.layers:
            x = layer(x, enc, self_bias, enc_bias)
        return x


class Transpeaker(nn.Module):
    """cfg: an object with h_dim, wemb, aemb, proj_hidden, speaker_layer_num, speaker_head_num, speaker_dropout, featdropout,
    image_feat_size, use_drop (the fields of M/r2r/parser.py:104-118 the reference reads at import time)."""

    def __init__(self, feature_size, hidden_size, word_size, tgt_vocab_size, cfg, padding_idx=0):
        super().__init__()
        self.encoder = TranspeakerEncoder(feature_size, hidden_size, cfg)
        self.decoder = TranspeakerDecoder(tgt_vocab_size, word_size, hidden_size, padding_idx, cfg)
        self.projection = nn.Linear(word_size, tgt_vocab_size, bias=False)
        self.dropout = nn.Dropout(cfg.speaker_dropout)
        self.use_drop = bool(getattr(cfg, 'use_drop', False))

    def forward(self, action_embeddings, world_state_embeddings, dec_inputs, ctx_mask=None, already_dropfeat=False):
        enc_inputs, enc_outputs = self.encoder(action_embeddings, world_state_embeddings, already_dropfeat)
        dec = self.decoder(dec_inputs, enc_outputs, ctx_mask)
        if self.use_drop:
            dec = hipops.dropout(dec, _p(self.dropout))
        return hipops.linear(dec, self.projection.weight, None, None, torch.float32)      # float32 logits [B, L, V]


def default_config(**over):
    from types import SimpleNamespace
    base = dict(h_dim=512, wemb=256, aemb=64, proj_hidden=1024, speaker_layer_num=3, speaker_head_num=4, speaker_dropout=0.2,
                featdropout=0.3, image_feat_size=768, speaker_angle_size=128, use_drop=False, maxDecode=120, attn_dropout_always=True)
    base.update(over)
    return SimpleNamespace(**base)


# ------------------------------------------------------------------------------------------------ the two uses (M/r2r/transpeaker.py)
def teacher_forcing_loss(model, can_feats, img_feats, insts, pad_id=0, ctx_mask=None):
    """M/r2r/transpeaker.py:233-239: cross-entropy of logits[:, :-1] against insts[:, 1:], <PAD> ignored, mean over the rest."""
    logits = model(can_feats, img_feats, insts, ctx_mask=ctx_mask)
    V = logits.shape[-1]
    return torch.nn.functional.cross_entropy(logits[:, :-1].reshape(-1, V), insts[:, 1:].reshape(-1).to(torch.int64), ignore_index=pad_id)


@torch.no_grad()
def infer_batch(model, can_feats, img_feats, bos, eos, pad, unk, max_decode=120, sampling=False, already_dropfeat=False):
    """M/r2r/transpeaker.py:248-318: encode once, then decode word by word (the decoder re-reads the whole prefix every step, as
    the reference does), <UNK> never produced, finished sentences padded; -> int64 [B, <= max_decode + 1] including <BOS>."""
    enc_inputs, enc_outputs = model.encoder(can_feats, img_feats, already_dropfeat)
    B = can_feats.shape[0]
    word = torch.full((B, 1), bos, dtype=torch.int64, device=can_feats.device)
    ended = torch.zeros(B, dtype=torch.bool, device=can_feats.device)
    for _ in range(max_decode):
        dec = model.decoder(word, enc_outputs)
        logits = hipops.linear(dec[:, -1:].contiguous(), model.projection.weight, None, None, torch.float32)[:, 0]
        logits[:, unk] = -float('inf')
        nxt = torch.distributions.Categorical(logits=logits).sample() if sampling else logits.argmax(-1)
        nxt = torch.where(ended, torch.full_like(nxt, pad), nxt)
        word = torch.cat([word, nxt.unsqueeze(1)], 1)
        ended = ended | (nxt == eos)
        if bool(ended.all()):
            break
    return word


# ------------------------------------------------------------------------------------------------ KV-cached, graph-replayed decoding
def _proj_cat(x, weights):
    """x @ cat(W_i)^T for bias-free Linears in one GEMM (the weights' concatenated shadow is cached and refreshed like every shadow)."""
    x2 = x.reshape(-1, x.shape[-1])
    if x2.shape[1] % 8 or not x2.is_contiguous():
        return torch.cat([hipops.linear(x, w) for w in weights], -1)
    W = hipops._shadow_cat(tuple(weights), x2.dtype)
    out = torch.empty((x2.shape[0], W.shape[0]), dtype=x2.dtype, device=x2.device)
    hipops.gemm(x2, W, out)
    return out.view(*x.shape[:-1], W.shape[0])


class IncrementalDecoder:
    """`TranspeakerDecoder` + projection + word choice, one token per row and step, on static state — so that a step is a fixed-shape
    computation: captured once (hipops.graph) after one eager warm-up step and replayed for every later word.

    Static state: per layer the self-attention K|V cache [B, max_decode + 1, 2*nh*64] (compute dtype; goat_attn_decode_fwd appends
    the step's row and attends over the rows written so far, the position read from device memory) and the cross-attention K|V of the
    encoder output [B, ctx_len, 2*nh*64], projected ONCE per sentence batch by `start`; hipops.DecodeState (words, kmask, ended,
    end_step, pos, n_live); the optional context bias [B, 1, ctx_len]; the float32 logits of the last step (`logits`).

        dec = IncrementalDecoder(model, B, max_decode, T)
        dec.start(enc_outputs, bos, pad, ctx_mask)             # new sentences
        dec.step(unk, eos, pad, sampling)                      # x max_decode; words in dec.state.words[:, :pos + 1]
        dec.force(next_words)                                  # (teacher forcing: replace the word the last step chose)

    Honours what TranspeakerDecoder / MultiHeadAttention honour: `use_drop`, `attn_dropout_always`, the compute dtype (fixed at
    construction), `ctx_mask`.  The step is a single-stream graph without parallel branches.

    Random numbers.  A captured step bakes in the (seed, offset) pairs RngState.next handed out at capture, so what makes a replay draw
    anew — dropout masks and, with `sampling`, the Gumbel noise of the word choice — is a device counter the step bumps itself.  The
    decoder owns that counter (`rng_dev=`: an int64 [1] tensor of the caller's instead, e.g. to share one among decoders); it is
    installed as hipops.RngState.dev only for the duration of a step and the process-wide value is put back afterwards, so decoding
    leaves the random streams of every other op as they were.  Eager stepping (use_graph=False) bumps it too, on top of the host
    offsets that advance anyway: eager and replayed steps are then different draws of the same distribution.

    Against the prefix form (`infer_batch`): at p = 0 both compute the same function.  With attention dropout active
    (`attn_dropout_always`, the reference's quirk) they are DIFFERENT RANDOM DRAWS of the same model: the prefix form re-draws the masks
    of every position at every step, the cached form draws a position's masks once, when that position is decoded (and the `use_drop`
    masks of the hoisted cross-attention K|V once per sentence batch)."""

    def __init__(self, model, B, max_decode, ctx_len, use_graph=True, rng_dev=None):
        dec = model.decoder
        dev = model.projection.weight.device
        self.model, self.B, self.max_decode, self.ctx_len = model, int(B), int(max_decode), int(ctx_len)
        self.dtype = compute_dtype()
        self.use_graph = use_graph
        self.state = hipops.DecodeState(B, max_decode + 1, dev)
        if rng_dev is not None and (rng_dev.dtype != torch.int64 or rng_dev.numel() != 1 or rng_dev.device != dev):
            raise ValueError('rng_dev is one int64 on the device of the model')
        self.rng_dev = rng_dev if rng_dev is not None else torch.zeros(1, dtype=torch.int64, device=dev)
        self.self_kv, self.cross_kv = [], []
        for layer in dec.layers:
            Hs, Hc = layer.dec_self_attn.W_K.weight.shape[0], layer.dec_enc_attn.W_K.weight.shape[0]
            self.self_kv.append(torch.zeros(B, max_decode + 1, 2 * Hs, dtype=self.dtype, device=dev))
            self.cross_kv.append(torch.zeros(B, ctx_len, 2 * Hc, dtype=self.dtype, device=dev))
        self.ctx_bias = torch.zeros(B, 1, ctx_len, dtype=torch.float32, device=dev)
        self.has_ctx_mask = False
        self.logits = torch.zeros(B, model.projection.weight.shape[0], dtype=torch.float32, device=dev)
        self._graphs = {}           # (unk, eos, pad, sampling, ctx mask in use, dropout probabilities) -> captured step
        self._warm = set()

    @staticmethod
    def _draws(probs):
        return any(probs[i] > 0 for i in (0, 1, 2, 4, 5, 6))

    # -- dropout probabilities at call time (they are baked into a captured step: part of the graph key)
    def _probs(self):
        m, d = self.model, self.model.decoder
        at = d.layers[0].dec_self_attn
        return (_p(d.drop) if d.use_drop else 0.0, _p(d.pos_emb.dropout), _p(at.dropout), bool(at.use_drop),
                at.attn_p if at.attn_p is not None else _p(at.dropout), _p(d.layers[0].pos_ffn.fc[2]),
                _p(m.dropout) if m.use_drop else 0.0)

    @torch.no_grad()
    def start(self, enc_outputs, first, pad=0, ctx_mask=None):
        """New sentences: hoist the cross-attention K|V of enc_outputs [B, ctx_len, hidden], reset the loop state with `first`
        (<BOS>, or int64 [B]) in column 0.  ctx_mask: bool [B, ctx_len] (True = padded context step) or None."""
        if tuple(enc_outputs.shape[:2]) != (self.B, self.ctx_len):
            raise ValueError('IncrementalDecoder built for [%d, %d] context steps, got %s' % (self.B, self.ctx_len, tuple(enc_outputs.shape[:2])))
        enc = enc_outputs.detach().to(self.dtype)
        for layer, kv in zip(self.model.decoder.layers, self.cross_kv):
            at = layer.dec_enc_attn
            x = _proj_cat(enc, (at.W_K.weight, at.W_V.weight))
            if at.use_drop:
                x = hipops.dropout(x, _p(at.dropout))
            kv.copy_(x)
        self.has_ctx_mask = ctx_mask is not None
        self.ctx_bias.zero_()
        if ctx_mask is not None:
            self.ctx_bias.masked_fill_(ctx_mask.bool().unsqueeze(1), -1e9)
        self.state.reset(first, pad)

    def _attn_out(self, at, ctx, x):
        out = at.ln(hipops.linear(ctx, at.fc.weight), x)
        return hipops.dropout(out, _p(at.dropout))

    def _step(self, unk, eos, pad, sampling):
        m, dec, st = self.model, self.model.decoder, self.state
        if sampling or self._draws(self._probs()):
            self.rng_dev.add_(0x9E3779B1)                       # a replay draws new masks and new Gumbel noise
        pos = st.pos.long()
        ids = st.words.index_select(1, pos)                                                     # [B, 1]
        x = hipops.embedding(ids, dec.embedding.weight, out_dtype=self.dtype, word_pad=dec.embedding.padding_idx)
        if dec.use_drop:
            x = hipops.dropout(x, _p(dec.drop))
        x = x + dec.pos_emb.pe[:, 0].index_select(0, pos).to(self.dtype).unsqueeze(0)
        x = hipops.dropout(x, _p(dec.pos_emb.dropout))
        for layer, skv, ckv in zip(dec.layers, self.self_kv, self.cross_kv):
            at = layer.dec_self_attn
            q = hipops.linear(x, at.W_Q.weight)                                                 # [B, 1, H]
            kv = _proj_cat(x, (at.W_K.weight, at.W_V.weight))                                   # [B, 1, 2H]: the row the cache gains
            if at.use_drop:
                q, kv = hipops.dropout(q, _p(at.dropout)), hipops.dropout(kv, _p(at.dropout))
            p = at.attn_p if at.attn_p is not None else _p(at.dropout)
            ctx = hipops.attn_decode(q, kv, skv, st.kmask, st.pos, at.n_heads, p)
            x = self._attn_out(at, ctx, x)
            at = layer.dec_enc_attn
            q = hipops.linear(x, at.W_Q.weight)
            if at.use_drop:
                q = hipops.dropout(q, _p(at.dropout))
            p = at.attn_p if at.attn_p is not None else _p(at.dropout)
            ctx = hipops.attention(q, ckv, None, self.ctx_bias if self.has_ctx_mask else None, at.n_heads, p)
            x = self._attn_out(at, ctx, x)
            x = layer.pos_ffn(x)
        if m.use_drop:
            x = hipops.dropout(x, _p(m.dropout))
        self.logits.copy_(hipops.linear(x, m.projection.weight, None, None, torch.float32)[:, 0])
        hipops.decode_select(self.logits, st, unk, eos, pad, sampling)

    @torch.no_grad()
    def step(self, unk, eos, pad=0, sampling=False):
        """Decode one word per row: state.words[:, pos + 1] is chosen and pos advances (on the device; nothing synchronises).  The first
        step of a configuration runs eagerly (the warm-up: weight shadows, GEMM configurations), the second is captured, every later
        one is a replay."""
        if compute_dtype() != self.dtype:
            raise RuntimeError('IncrementalDecoder was built for %s; the compute dtype is now %s' % (self.dtype, compute_dtype()))
        probs = self._probs()
        key = (int(unk), int(eos), int(pad), bool(sampling), self.has_ctx_mask, probs)
        g = self._graphs.get(key)
        if g is None:
            outer, hipops.RngState.dev = hipops.RngState.dev, self.rng_dev      # (the ops of the step take the counter's address from here)
            try:
                if not self.use_graph or key not in self._warm:
                    self._warm.add(key)
                    return self._step(unk, eos, pad, sampling)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with hipops.graph(g):
                    self._step(unk, eos, pad, sampling)
                self._graphs[key] = g
            finally:
                hipops.RngState.dev = outer
        g.replay()

    @torch.no_grad()
    def force(self, next_words, pad=0):
        """Teacher forcing: replace the word the last step chose (column pos) by next_words int64 [B]; its key mask follows."""
        pos = self.state.pos.long()
        w = next_words.to(torch.int64).reshape(self.B, 1)
        self.state.words.index_copy_(1, pos, w)
        self.state.kmask.index_copy_(1, pos, torch.zeros_like(w, dtype=torch.float32).masked_fill_(w == pad, -1e9))


@torch.no_grad()
def infer_batch_cached(model, can_feats, img_feats, bos, eos, pad, unk, max_decode=120, sampling=False, already_dropfeat=False,
                       ctx_mask=None, check_every=8, decoder=None):
    """`infer_batch` with a KV cache and a captured step (IncrementalDecoder): encode once, hoist the cross-attention K|V once, then
    one graph replay per word; the only device-to-host reads are n_live once every `check_every` steps and end_step at the end.
    Same result contract: int64 [B, <= max_decode + 1] including <BOS>, cut where the last row ended (1 + max(end_step) + 1 columns),
    <UNK> never produced, finished rows padded.  decoder=: reuse one IncrementalDecoder (and its captured graph) across batches of the
    same B, max_decode and context length.

    At p = 0 this is the function `infer_batch` computes.  With attention dropout active (`attn_dropout_always`, the reference's quirk)
    the two are different random draws: the prefix form re-draws every position's masks at every step, this form draws a position's
    masks once, when that position is decoded."""
    enc_inputs, enc_outputs = model.encoder(can_feats, img_feats, already_dropfeat)
    B, T = enc_outputs.shape[0], enc_outputs.shape[1]
    dec = decoder if decoder is not None else IncrementalDecoder(model, B, max_decode, T)
    if (dec.B, dec.max_decode, dec.ctx_len) != (B, max_decode, T) or dec.model is not model:
        raise ValueError('decoder= was built for another model or (B, max_decode, ctx_len) = (%d, %d, %d)' % (dec.B, dec.max_decode, dec.ctx_len))
    dec.start(enc_outputs, bos, pad, ctx_mask)
    check_every = max(1, int(check_every))
    for s in range(max_decode):
        dec.step(unk, eos, pad, sampling)
        if (s + 1) % check_every == 0 and s + 1 < max_decode and int(dec.state.n_live.item()) == 0:
            break
    st = dec.state
    n = max_decode + 1 if int(st.n_live.item()) else int(st.end_step.max().item()) + 2
    return st.words[:, :n].clone()


# ------------------------------------------------------------------------------------------------ back-translation (M/r2r/agent.py:457-474)
def shrink_words(row, bos, eos):
    """`Tokenizer.shrink` (M/utils/data.py:373-398) on a plain list of word ids, quirks included:
      * w[i] is kept only where w[i] != w[i + 1], for i < len - 1: the LAST column is always dropped, a run collapses to its last element
        and a trailing run (the <PAD> tail, and a final <EOS> in front of nothing) disappears whole;
      * end = index of the first <EOS> among the kept words — np.argmax of the comparison, which is 0 both when there is none and when
        <EOS> comes first; either way end becomes the number of kept words ([<EOS>, a, b] keeps its <EOS>; a row without <EOS> loses
        nothing but its last column);
      * the first kept word is dropped if it is <BOS> and is not the only one ([<BOS>, <EOS>] decodes to '<BOS>').
    An empty row comes back empty.  A row of one element, and a row that is one run of a single word, leave nothing to look for <EOS>
    in: the reference's np.argmax raises ValueError there, and so does this."""
    row = [int(w) for w in row]
    if not row:
        return row
    kept = [row[i] for i in range(len(row) - 1) if row[i] != row[i + 1]]
    if not kept:
        raise ValueError('shrink_words: nothing is kept of a row of %d equal words (the reference raises: argmax of an empty sequence)' % len(row))
    end = kept.index(eos) if eos in kept else 0
    if end == 0:
        end = len(kept)
    start = 1 if (len(kept) > 1 and kept[0] == bos) else 0
    return kept[start:end]


def decode_words(row, pad):
    """`Tokenizer.decode_sentence` (M/utils/data.py:362-371) without the join: the words up to the first <PAD>."""
    out = []
    for w in row:
        if int(w) == pad:
            break
        out.append(int(w))
    return out


class RetokTable:
    """The agent's tokenizer restricted to what the speaker can say: per speaker word the agent ids of the word at the start of a
    sentence (`encode(w)`) and behind a space (`encode(' ' + w)`; a byte-level BPE tokenises "walk" and " walk" differently), as two CSR
    tables of int32 device tensors: first_start / rest_start [V + 1], first_ids / rest_ids.  goat_retok_rows expands words through them.

    It rests on one assumption: the tokenizer never merges across the single spaces `decode_sentence` joins the words with, so that a
    sentence's tokenisation is the concatenation of its words'.  `check` verifies it for given sentences."""

    def __init__(self, vocab_words, first, rest, device=None):
        if len(first) != len(vocab_words) or len(rest) != len(vocab_words) or not vocab_words:
            raise ValueError('RetokTable: one id list per vocabulary word and place')
        self.vocab = list(vocab_words)
        self.V = len(self.vocab)
        self.first = [[int(i) for i in ids] for ids in first]
        self.rest = [[int(i) for i in ids] for ids in rest]
        if device is None:
            device = 'cuda' if torch.cuda.is_available() else 'cpu'
        for name, lists in (('first', self.first), ('rest', self.rest)):
            start = np.zeros(self.V + 1, np.int64)
            start[1:] = np.cumsum([len(ids) for ids in lists])
            flat = np.asarray([i for ids in lists for i in ids] or [0], np.int64)      # (never empty: a pointer to hand to the kernel)
            if start[-1] >= 2 ** 31 or flat.min() < -2 ** 31 or flat.max() >= 2 ** 31:
                raise ValueError('RetokTable: ids and offsets are int32')
            setattr(self, name + '_start', torch.from_numpy(start.astype(np.int32)).to(device))
            setattr(self, name + '_ids', torch.from_numpy(flat.astype(np.int32)).to(device))

    @classmethod
    def build(cls, vocab_words, encode, device=None):
        """vocab_words: the speaker vocabulary in id order, <BOS> included; encode: str -> list[int] WITHOUT special tokens (for the
        reference's agent: lambda s: tok(s, add_special_tokens=False)['input_ids'])."""
        return cls(vocab_words, [encode(w) for w in vocab_words], [encode(' ' + w) for w in vocab_words], device)

    def host(self, words):
        """the expansion goat_retok_rows makes, in Python: agent ids of the sentence `words` (speaker ids), no special tokens"""
        out = []
        for j, w in enumerate(words):
            out += (self.first if j == 0 else self.rest)[int(w)]
        return out

    def sentence(self, words):
        return ' '.join(self.vocab[int(w)] for w in words)

    def instr_encoding(self, row, bos, eos, pad, agent_bos, agent_eos, max_len=None):
        """a row of decoded words -> the `instr_encoding` the reference resets its environment with: shrink, decode_sentence, tokenise,
        `[:max_len]` — a plain slice, which loses the </s> of a sentence that is too long (M/r2r/agent.py:934)."""
        ids = [int(agent_bos)] + self.host(decode_words(shrink_words(row, bos, eos), pad)) + [int(agent_eos)]
        return ids if max_len is None else ids[:max_len]

    def check(self, encode, sentences):
        """Raise ValueError when, for one of `sentences` (lists of speaker word ids), the tokenisation of the whole joined string is not
        the concatenation of the table's per-word ids."""
        for words in sentences:
            text = self.sentence(words)
            whole, parts = [int(i) for i in encode(text)], self.host(words)
            if whole != parts:
                raise ValueError('RetokTable: the tokenizer merges across words: %r encodes to %s, word by word to %s' % (text, whole, parts))


class BackTranslator:
    """Speaker words to agent instruction without leaving the device: what the reference's self-training rollout does between
    `speaker.infer_batch` and `env.reset_epoch` (M/r2r/agent.py:457-474) — one shared environment-dropout mask on the speaker's image
    features, greedy / sampled decoding, shrink + decode_sentence + the agent's tokenizer — with the KV-cached decoder and one
    goat_retok_rows launch that writes the agent's `txt_ids` / `txt_masks` in place.

        bt = BackTranslator(model, table, B, max_decode, T, bos, eos, pad, unk, agent_bos, agent_eos)
        bt.draw_noise(vln_bert)                                        # noise = drop_env(ones(D)), in bt.noise
        bt.run(can_feats, img_feats, bufs.t['txt_ids'], bufs.t['txt_masks'], noise=bt.noise)
        nav.walk(ep, episodes, ..., text='device')                     # and extras={'panorama': {'env_noise': bt.noise}} in the body

    run() makes no host read beyond the decoder's own n_live check; a row the reference would have raised on is recorded in
    `status` and raised by check() / instr_encodings(), which synchronise."""

    def __init__(self, model, table, B, max_decode, ctx_len, bos, eos, pad, unk, agent_bos, agent_eos, fill_id=0):
        self.model, self.table = model, table
        self.decoder = IncrementalDecoder(model, B, max_decode, ctx_len)
        self.B, self.max_decode, self.ctx_len = int(B), int(max_decode), int(ctx_len)
        self.bos, self.eos, self.pad, self.unk = int(bos), int(eos), int(pad), int(unk)
        self.agent_bos, self.agent_eos, self.fill_id = int(agent_bos), int(agent_eos), int(fill_id)
        if table.V != model.projection.weight.shape[0]:
            raise ValueError('BackTranslator: the table holds %d words, the speaker projects onto %d' % (table.V, model.projection.weight.shape[0]))
        dev = model.projection.weight.device
        self.D = int(model.encoder.image_feat_size)
        self.noise = torch.ones(self.D, dtype=torch.float32, device=dev)
        self.lens = torch.zeros(B, dtype=torch.int32, device=dev)
        self.status = torch.zeros(B, dtype=torch.int32, device=dev)
        self.out_ids = None

    @torch.no_grad()
    def draw_noise(self, vln_bert):
        """noise = vln_bert.drop_env(ones(D)) (M/r2r/agent.py:459) into the persistent buffer: all ones in eval mode."""
        self.noise.copy_(hipops.dropout(torch.ones_like(self.noise), _p(vln_bert.drop_env)))
        return self.noise

    def _scaled(self, x, noise):
        x = x.detach()
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()
        return hipops.scale_cols(x.contiguous(), noise)

    @torch.no_grad()
    def run(self, can_feats, img_feats, out_ids, out_masks, noise=None, sampling=False, check_every=8, max_len=None):
        """can_feats [B, T, F], img_feats [B, T, 36, F] (speaker.path_features) -> the instruction rows in out_ids int64 / out_masks bool
        [B, L] (e.g. the `txt_ids` / `txt_masks` of an EpisodeBuffers), at most max_len (default L) tokens each; -> lens int32 [B] on
        the device.  noise: float32 [D] multiplied into the image columns of both inputs (transpeaker.py:272-278), the encoder then
        skips its own feature dropout; None: the encoder drops per element as `infer_batch_cached` does."""
        if noise is not None:
            can_feats, img_feats = self._scaled(can_feats, noise), self._scaled(img_feats, noise)
        enc_inputs, enc_outputs = self.model.encoder(can_feats, img_feats, noise is not None)
        dec = self.decoder
        dec.start(enc_outputs, self.bos, self.pad)
        check_every = max(1, int(check_every))
        for s in range(self.max_decode):
            dec.step(self.unk, self.eos, self.pad, sampling)
            if (s + 1) % check_every == 0 and s + 1 < self.max_decode and int(dec.state.n_live.item()) == 0:
                break
        hipops.retok_rows(dec.state.words, self.table, out_ids, out_masks, self.bos, self.eos, self.pad, self.agent_bos, self.agent_eos,
                          self.fill_id, max_len, state=dec.state, lens=self.lens, status=self.status, check=False)
        layers.refresh_masks(only=[out_masks, out_ids], force=True)      # (a raw kernel write bumps no version counter)
        self.out_ids = out_ids
        return self.lens

    def check(self):
        """raise ValueError for a row of the last run the reference would have raised on (reads the status back)"""
        hipops.check_retok_status(self.status)

    def instr_encodings(self):
        """the instructions of the last run as lists of agent ids (`episodes[i]['instr_encoding']` of the host-planner forms); this is a
        read-back."""
        if self.out_ids is None:
            raise RuntimeError('BackTranslator.instr_encodings: nothing has run')
        self.check()
        ids, lens = self.out_ids.cpu(), self.lens.cpu().tolist()
        return [ids[i, :lens[i]].tolist() for i in range(self.B)]


def path_features(sim, store, episodes, angle_size=128):
    """`from_shortest_path` (M/r2r/transpeaker.py:158-199) on the graph-only navigator: walk every ground-truth path; per step the
    36 view features + their relative angle features (`speaker_feature` of the observation, M/r2r/env.py:362-364) and the feature of
    the view in which the next viewpoint is seen (zeros at the stop step).  -> (img_feats [B, T, 36, F], can_feats [B, T, F]
    float32 on the store's device, lengths [B])."""
    from . import navsim
    obs = sim.reset(episodes)
    B = len(obs)
    D = store.table.shape[1]
    F = D + angle_size
    table = navsim.view_angle_feature_table(angle_size)
    ended = np.zeros(B, bool)
    lengths = np.zeros(B, np.int64)
    rows, angs, crow, cang = [], [], [], []
    while not ended.all():
        r = np.stack([ob['feature_row'] * 36 + np.arange(36) for ob in obs])
        a = np.stack([table[ob['viewIndex']] for ob in obs])
        cr = np.full(B, -1, np.int64)
        ca = np.zeros((B, angle_size), np.float32)
        moves = []
        for i, ob in enumerate(obs):
            path = ob['gt_path']
            nxt = None
            if not ended[i] and ob['viewpoint'] in path:
                k = path.index(ob['viewpoint'])
                nxt = path[k + 1] if k + 1 < len(path) else None
            if nxt is None:
                moves.append(None)
            else:
                c = next(c for c in ob['candidate'] if c['viewpointId'] == nxt)
                cr[i] = ob['feature_row'] * 36 + c['pointId']
                ca[i] = navsim.angle_feature(c['heading'], c['elevation'], angle_size)
                moves.append((nxt, c['pointId']))
        rows.append(r)
        angs.append(a)
        crow.append(cr)
        cang.append(ca)
        lengths += (~ended)
        ended = np.logical_or(ended, np.array([m is None for m in moves]))
        obs = sim.step(moves)
    dev = store.dev.device
    rows_t = torch.from_numpy(np.stack(rows, 1)).to(dev)                       # [B, T, 36]
    img = torch.cat([store.gather(rows_t).float(), torch.from_numpy(np.stack(angs, 1)).to(dev)], -1)
    crow_t = torch.from_numpy(np.stack(crow, 1)).to(dev)                       # [B, T], -1 at the stop step
    can = torch.cat([store.gather(crow_t).float(), torch.from_numpy(np.stack(cang, 1)).to(dev)], -1)
    return img, can, lengths
