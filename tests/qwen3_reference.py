"""Float64 restatement, in plain torch, of the Qwen3 text decoder that mlx8_ws_audio_transformer_amd.music2midi.Qwen3Decoder runs on libawt, of its four
operators, and of the reference's generate loop (.charles/music2midi/model.py:293-344).  No tests here; `transformers` is not needed (tests/
test_qwen3_reference_host.py compares this file with `Qwen3ForCausalLM` where that package exists).

    rmsnorm / qk_norm_rope / silu_mul / causal_attention    `exact` per-operator functions, float64
    rounded_causal_attention                                tests/cross_attention_reference.py's forward roundings with the causal bound and grouped KV heads
    state_dict(cfg, seed), variates(...)                    weights and inputs from the project's counter-based variates: the same bits on every machine
    forward(sd, cfg, x), causal_lm_loss(logits, labels)     the decoder and HF's shifted loss
    greedy(...)                                             the reference's full-recompute loop: adapter over the whole text each step, no cache

Scales: linears 1.5 / sqrt(fan_in), norm gains 1 + 0.3 N(0, 1), embeddings N(0, 1); every value is rounded to fp32 first, so the module under test and
this file hold the same numbers.  The rotary tables are HF's: fp32 inv_freq, fp32 outer product with the position, then cos / sin (they are part of the
model's definition, so the restatement uses the fp32 tables, in float64 arithmetic)."""
import numpy as np
import torch

from mlx8_ws_audio_transformer_amd import weights as wts
from mlx8_ws_audio_transformer_amd.music2midi import Qwen3Config
from tests import cross_attention_reference as xr

D = 128
MICRO = dict(vocab_size=320, hidden_size=256, intermediate_size=384, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, rms_norm_eps=1e-6,
             rope_theta=1e6, max_position_embeddings=1024)
WIDE = dict(vocab_size=1000, hidden_size=1024, intermediate_size=3072, num_hidden_layers=1, num_attention_heads=16, num_key_value_heads=8, rms_norm_eps=1e-6,
            rope_theta=1e6, max_position_embeddings=1024)


def config(base, tied):
    return Qwen3Config(tie_word_embeddings=tied, **base)


def variates(name, shape, seed, scale=1.0):
    """float64 tensor of fp32-representable values."""
    u = torch.from_numpy(wts.unit_variates(name, int(np.prod(shape)), seed).reshape(shape)).double() * scale
    return u.float().double()


def parameter_shapes(cfg):
    d, I, Hq, Hkv = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.num_key_value_heads
    shapes = {"model.embed_tokens.weight": (cfg.vocab_size, d), "model.norm.weight": (d,)}
    for n in range(cfg.num_hidden_layers):
        p = f"model.layers.{n}."
        shapes.update({p + "self_attn.q_proj.weight": (Hq * D, d), p + "self_attn.k_proj.weight": (Hkv * D, d), p + "self_attn.v_proj.weight": (Hkv * D, d),
                       p + "self_attn.o_proj.weight": (d, Hq * D), p + "self_attn.q_norm.weight": (D,), p + "self_attn.k_norm.weight": (D,),
                       p + "mlp.gate_proj.weight": (I, d), p + "mlp.up_proj.weight": (I, d), p + "mlp.down_proj.weight": (d, I),
                       p + "input_layernorm.weight": (d,), p + "post_attention_layernorm.weight": (d,)})
    if not cfg.tie_word_embeddings:
        shapes["lm_head.weight"] = (cfg.vocab_size, d)
    return shapes


def state_dict(cfg, seed):
    sd = {}
    for name, shape in parameter_shapes(cfg).items():
        u = variates("qwen3." + name, shape, seed)
        if "norm" in name:
            sd[name] = (1.0 + 0.3 * u).float().double()
        elif "embed_tokens" in name:
            sd[name] = u
        else:
            sd[name] = (1.5 * shape[1] ** -0.5 * u).float().double()
    return sd


def rope_tables(theta, rows):
    """(cos, sin) fp32 [rows, 64], HF's Qwen3RotaryEmbedding arithmetic on the host."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.int64).to(dtype=torch.float32) / D))
    ang = torch.arange(rows, dtype=torch.float32)[:, None] * inv_freq[None, :]
    return ang.cos(), ang.sin()


# ------------------------------------------------------------------------------------------------ operators, exact
def rmsnorm(x, gamma, eps):
    x = x.double()
    return gamma.double() * x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)


def rotate(x, cos, sin):
    """x [..., 128] with cos / sin [..., 64] broadcastable: x cos + rotate_half(x) sin, dim i paired with i + 64."""
    a, b = x[..., :64], x[..., 64:]
    return torch.cat([a * cos - b * sin, b * cos + a * sin], dim=-1)


def qk_norm_rope(qkv, q_gamma, k_gamma, cos, sin, positions, Hq, Hkv, eps):
    """qkv [rows, (Hq + 2 Hkv) 128], positions [rows] -> q [rows, Hq, 128], k [rows, Hkv, 128] (normed, then rotated), v [rows, Hkv, 128] (untouched)."""
    rows_ = qkv.shape[0]
    x = qkv.double().view(rows_, Hq + 2 * Hkv, D)
    c, s = cos.double()[positions.long()][:, None, :], sin.double()[positions.long()][:, None, :]
    q = rotate(rmsnorm(x[:, :Hq], q_gamma, eps), c, s)
    k = rotate(rmsnorm(x[:, Hq:Hq + Hkv], k_gamma, eps), c, s)
    return q, k, x[:, Hq + Hkv:]


def silu_mul(gu, I):
    g, u = gu.double()[..., :I], gu.double()[..., I:2 * I]
    return g / (1.0 + torch.exp(-g)) * u


def causal_mask(Lq, T, device=None):
    """[Lq, T] bool: query i sees key j iff j <= T - Lq + i."""
    return torch.arange(T, device=device)[None, :] <= (T - Lq) + torch.arange(Lq, device=device)[:, None]


def causal_attention(q, k, v):
    """q [B, Hq, Lq, 128], k / v [B, Hkv, T, 128] -> o [B, Hq, Lq, 128], float64; query head h reads KV head h / (Hq / Hkv)."""
    g = q.shape[1] // k.shape[1]
    k, v = k.double().repeat_interleave(g, dim=1), v.double().repeat_interleave(g, dim=1)
    s = q.double() @ k.transpose(2, 3) * D ** -0.5
    s = s.masked_fill(~causal_mask(q.shape[2], k.shape[2], q.device), float("-inf"))
    return torch.softmax(s, dim=-1) @ v


def rounded_causal_attention(q, k, v, terms=3):
    """The forward of cross_attention_reference.rounded with the causal bound and the head grouping: the same roundings and nothing else.  A masked score
    is -1e30 as in the kernel; a tile that lies wholly past a row's diagonal leaves that row's running state unchanged (alpha = 1, p = 0), which is what
    skipping the tile does."""
    B, Hq, Lq, _ = q.shape
    g, T = Hq // k.shape[1], k.shape[2]
    k, v = k.repeat_interleave(g, dim=1), v.repeat_interleave(g, dim=1)
    qh, ql = xr._split(q, terms)
    kh, kl = xr._split(k, terms)
    vh, vl = xr._split(v, terms)
    sc2 = float(torch.tensor(xr.SCALE, dtype=torch.float32) * torch.tensor(xr.LOG2E, dtype=torch.float32))
    s = torch.zeros((B, Hq, Lq, T), dtype=torch.float64, device=q.device)
    for c in range(0, D, 16):
        a_h, a_l, b_h, b_l = qh[..., c:c + 16], ql[..., c:c + 16], kh[..., c:c + 16].transpose(2, 3), kl[..., c:c + 16].transpose(2, 3)
        if terms == 3:
            s = xr._f32(s + a_h @ b_l)
            s = xr._f32(s + a_l @ b_h)
        s = xr._f32(s + a_h @ b_h)
    s2 = xr._f32(s * sc2).masked_fill(~causal_mask(Lq, T, q.device), -1.0e30)
    m = torch.full((B, Hq, Lq), -1.0e30, dtype=torch.float64, device=q.device)
    l = torch.zeros_like(m)
    acc = torch.zeros((B, Hq, Lq, D), dtype=torch.float64, device=q.device)
    for t0 in range(0, T, xr.KEY_TILE):
        st = s2[..., t0:t0 + xr.KEY_TILE]
        m_new = torch.maximum(m, st.max(-1).values)
        alpha = xr._f32(torch.exp2(m - m_new))
        p = xr._f32(torch.exp2(st - m_new[..., None]))
        l = xr._f32(l * alpha + p.sum(-1))
        ph, pl = xr._split(p, terms)
        acc = xr._f32(acc * alpha[..., None] + xr._prod(ph, pl, vh[..., t0:t0 + xr.KEY_TILE, :], vl[..., t0:t0 + xr.KEY_TILE, :], terms))
        m = m_new
    return xr._f32(acc * xr._f32(1.0 / l)[..., None])


# ------------------------------------------------------------------------------------------------ the decoder
def forward(sd, cfg, x):
    """inputs_embeds x [B, L, hidden] -> logits [B, L, vocab], float64 (positions 0 .. L - 1, causal mask only)."""
    B, L, d = x.shape
    Hq, Hkv, I, eps = cfg.num_attention_heads, cfg.num_key_value_heads, cfg.intermediate_size, cfg.rms_norm_eps
    W = lambda name: sd[name].double().to(x.device)
    cos, sin = (t.to(x.device) for t in rope_tables(cfg.rope_theta, L))
    positions = torch.arange(L, device=x.device).repeat(B)
    x = x.double().reshape(B * L, d)
    for n in range(cfg.num_hidden_layers):
        p = f"model.layers.{n}."
        h = rmsnorm(x, W(p + "input_layernorm.weight"), eps)
        qkv = h @ torch.cat([W(p + "self_attn.q_proj.weight"), W(p + "self_attn.k_proj.weight"), W(p + "self_attn.v_proj.weight")]).T
        q, k, v = qk_norm_rope(qkv, W(p + "self_attn.q_norm.weight"), W(p + "self_attn.k_norm.weight"), cos, sin, positions, Hq, Hkv, eps)
        heads = lambda t: t.reshape(B, L, -1, D).permute(0, 2, 1, 3)
        o = causal_attention(heads(q), heads(k), heads(v)).permute(0, 2, 1, 3).reshape(B * L, Hq * D)
        x = x + o @ W(p + "self_attn.o_proj.weight").T
        h = rmsnorm(x, W(p + "post_attention_layernorm.weight"), eps)
        gu = h @ torch.cat([W(p + "mlp.gate_proj.weight"), W(p + "mlp.up_proj.weight")]).T
        x = x + silu_mul(gu, I) @ W(p + "mlp.down_proj.weight").T
    head = W("model.embed_tokens.weight") if cfg.tie_word_embeddings else W("lm_head.weight")
    return (rmsnorm(x, W("model.norm.weight"), eps) @ head.T).reshape(B, L, -1)


def causal_lm_loss(logits, labels):
    """HF's ForCausalLMLoss: logits at t against the label at t + 1, ignore_index -100, mean over the counted positions."""
    lg, lb = logits[:, :-1].reshape(-1, logits.shape[-1]).double(), labels[:, 1:].reshape(-1).to(logits.device)
    return torch.nn.functional.cross_entropy(lg, lb, ignore_index=-100)


def greedy(sd, cfg, adapter, audio, prompt, steps, eos=None):
    """The reference's loop with argmax for its multinomial: every step embeds the WHOLE text, runs the adapter over it against the audio features and the
    decoder over the result, no cache.  adapter: a float64 tests/music2midi_reference.ReferenceAdapter; audio [1, Sa, audio_dim].  Returns (tokens, per-step
    last-position logits [steps, vocab])."""
    ids, out, rows_ = list(prompt), [], []
    with torch.no_grad():
        for _ in range(steps):
            text = sd["model.embed_tokens.weight"].double().to(audio.device)[torch.tensor(ids, device=audio.device)][None]
            logits = forward(sd, cfg, adapter(text, audio.double()))[0, -1]
            rows_.append(logits)
            nxt = int(logits.argmax())
            if eos is not None and nxt == eos:
                break
            out.append(nxt)
            ids.append(nxt)
    return out, torch.stack(rows_)


# ------------------------------------------------------------------------------------------------ the greedy-generation fixture
GREEDY_SEED = 396                     # the first seed at which the conditions of tests/test_qwen3_reference_host.py hold (checked there, from this file alone)
GREEDY_STEPS = 24
GREEDY_PROMPTS = ([5], [17, 42, 3])
GREEDY_EOS = 319                      # never the argmax in the fixture's 24 steps (asserted by the host test): the loop runs its full length


def greedy_fixture(seed=GREEDY_SEED):
    """(cfg, state dict, float64 reference adapter, audio features [1, 130, 128]) of the greedy-generation test: the untied micro decoder (with tied N(0, 1)
    embeddings the model repeats its input token), an adapter of 2 heads over text_dim 256, seeded audio features."""
    from tests.music2midi_reference import ReferenceAdapter, nontrivial_
    cfg = config(MICRO, tied=False)
    adapter = nontrivial_(ReferenceAdapter(128, cfg.hidden_size, num_heads=2), seed).eval()
    return cfg, state_dict(cfg, seed), adapter, variates("qwen3.audio", (1, 130, 128), seed)
