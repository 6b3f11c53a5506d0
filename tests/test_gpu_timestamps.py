"""GPU: awt_op_select_tokens_ts -- token selection with Whisper's timestamp rules -- against a torch restatement of HF's
SuppressTokensAtBegin / SuppressTokens / WhisperTimeStampLogitsProcessor (transformers/generation/logits_process.py)."""
import numpy as np
import pytest
import torch

from mlx8_ws_audio_transformer_amd import generation as G

pytestmark = pytest.mark.gpu

LAYOUTS = {51865: 50363, 51866: 50364}          # vocab -> <|notimestamps|> (timestamp_begin = + 1)
EOS = {51865: 50257, 51866: 50257}


def _hf_rules(x, hist, begin, cur_len, eos, no_ts, mii, banned, log_softmax):
    """HF's processors in order on [rows, vocab] scores; log_softmax first for beam search (HF's _beam_search)."""
    tb = no_ts + 1
    s = torch.log_softmax(x.double().float(), dim=-1) if log_softmax else x.clone()
    if banned:
        s[:, list(banned)] = float("-inf")
    s[:, no_ts] = float("-inf")
    for k in range(s.shape[0]):
        seq = hist[k, begin:cur_len].tolist()
        last = len(seq) >= 1 and seq[-1] >= tb
        pen = len(seq) < 2 or seq[-2] >= tb
        if last:
            if pen:
                s[k, tb:] = float("-inf")
            else:
                s[k, :eos] = float("-inf")
        stamps = [t for t in seq if t >= tb]
        if stamps:
            lim = stamps[-1] if (last and not pen) else stamps[-1] + 1
            s[k, tb:lim] = float("-inf")
    if cur_len == begin:
        s[:, :tb] = float("-inf")
        if mii is not None:
            s[:, tb + mii + 1:] = float("-inf")
    lp = torch.log_softmax(s.float(), dim=-1)
    for k in range(s.shape[0]):
        if lp[k, tb:].logsumexp(dim=-1) > lp[k, :tb].max():
            s[k, :tb] = float("-inf")
    return s


def _reference(s, beams, bs, k, vocab):
    if bs is not None:
        s = s + bs[:, None]
    flat = s.reshape(-1, beams * vocab)
    vals, idx = torch.sort(flat, dim=1, descending=True, stable=True)
    return vals[:, :k], idx[:, :k] % vocab, (idx[:, :k] // vocab).to(torch.int32)


def _history(rows, begin, cur_len, tb, vocab, branch, g):
    """Token histories (prompt of `begin` tokens, then generated tokens) that put every row in the rule branch `branch`."""
    h = torch.randint(0, tb - 100, (rows, cur_len + 3), generator=g)
    h[:, :begin] = 50258
    gen = cur_len - begin
    for r in range(rows):
        ts = lambda: int(tb + torch.randint(0, 1400, (1,), generator=g))
        if branch == "text_text" and gen >= 1:
            if gen >= 3:
                h[r, begin] = tb + 20
        elif branch == "text_ts" and gen >= 2:
            h[r, cur_len - 1] = ts()
        elif branch == "ts_ts" and gen >= 2:
            a = ts()
            h[r, cur_len - 2], h[r, cur_len - 1] = a, a + 3
        elif branch == "lone_ts" and gen >= 1:
            h[r, cur_len - 1] = ts() if gen == 1 else h[r, cur_len - 1]
            if gen >= 1:
                h[r, begin:cur_len] = torch.randint(0, tb - 100, (gen,), generator=g)
                h[r, begin] = ts()
                if gen >= 2:
                    h[r, cur_len - 1] = h[r, begin]        # text ... then a timestamp equal to the first (monotonic rule: >= it)
        elif branch == "mixed":
            pick = r % 4
            if pick == 1 and gen >= 2:
                h[r, cur_len - 1] = ts()
            elif pick == 2 and gen >= 2:
                a = ts(); h[r, cur_len - 2], h[r, cur_len - 1] = a, a + 1
            elif pick == 3 and gen >= 3:
                h[r, begin + 1] = ts()
    return h


@pytest.mark.parametrize("vocab", [51865, 51866])
@pytest.mark.parametrize("beams", [1, 5, 8])
@pytest.mark.parametrize("branch", ["first", "first_mii", "text_text", "text_ts", "ts_ts", "lone_ts", "mixed"])
def test_select_tokens_ts_matches_hf_processors(vocab, beams, branch):
    no_ts = LAYOUTS[vocab]
    tb, eos = no_ts + 1, EOS[vocab]
    g = torch.Generator().manual_seed(vocab + 31 * beams + len(branch))
    clips = 3
    rows = clips * beams
    begin = 4
    cur_len = begin if branch.startswith("first") else begin + 6
    mii = 50 if branch == "first_mii" else None
    hist = _history(rows, begin, cur_len, tb, vocab, branch, g)
    ld = vocab + (-vocab) % 128
    x = torch.randn((rows, ld), generator=g) * 3
    x[:, tb:vocab] += torch.linspace(-2.0, 2.5, rows)[:, None]       # rows on both sides of the forcing rule
    x[:, vocab:] = 1e4
    x = x.cuda()
    banned = [eos, 50358, 50359, 50360, 50361, 50362, 220] if cur_len == begin else [50358, 50359, 50360, 50361, 50362]
    bits = G.banned_bits(banned, vocab, "cuda")
    bs = torch.randn(rows, generator=g).cuda() * 2 if beams > 1 else None
    rules = G.TimestampRules(eos, no_ts, begin, mii)
    hist_d = hist.cuda()
    for log_softmax, k in (((False, 1),) if beams == 1 else ((True, 2 * beams),)):
        got = G.select_tokens(x, vocab, beams, bits, bs, log_softmax, k, rules=rules, history=hist_d, cur_len=cur_len)
        s = _hf_rules(x[:, :vocab].cpu(), hist, begin, cur_len, eos, no_ts, mii, banned, log_softmax)
        ref = _reference(s, beams, None if bs is None else bs.cpu(), k, vocab)
        fin = torch.isfinite(ref[0])
        assert torch.equal(torch.isfinite(got[0].cpu()), fin)
        np.testing.assert_array_equal(got[1].cpu()[fin].numpy(), ref[1][fin].numpy())
        np.testing.assert_array_equal(got[2].cpu()[fin].numpy(), ref[2][fin].numpy())
        torch.testing.assert_close(got[0].cpu()[fin], ref[0][fin], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("vocab", [51865, 51866])
def test_select_tokens_ts_nan_inf_and_all_banned_rows(vocab):
    no_ts = LAYOUTS[vocab]
    tb, eos = no_ts + 1, EOS[vocab]
    begin, cur_len = 3, 8
    ld = vocab + (-vocab) % 128
    x = torch.randn((5, ld)) * 2
    x[0, 1234] = float("nan")                                        # NaN text: wins argmax, forcing rule does not fire
    x[1, tb + 700] = float("nan")                                    # NaN timestamp: no forcing, NaN chosen
    x[2, :vocab] = float("-inf")                                     # all -inf: index 0
    x[3, :tb] = float("-inf")                                        # only timestamps finite: forced, a timestamp
    x[4, tb:vocab] = 30.0                                            # timestamps dominate, but the history bans them all
    hist = torch.randint(0, 1000, (5, cur_len))
    hist[:, :begin] = 50258
    hist[4, cur_len - 2], hist[4, cur_len - 1] = tb + 5, tb + 9      # two timestamps: timestamps banned
    rules = G.TimestampRules(eos, no_ts, begin, None)
    got = G.select_tokens(x.cuda(), vocab, 1, None, None, False, 1, rules=rules, history=hist.cuda(), cur_len=cur_len)[1][:, 0].cpu()
    s = _hf_rules(x[:, :vocab], hist, begin, cur_len, eos, no_ts, None, [], False)
    ref = s.argmax(dim=-1)
    assert got.tolist() == ref.tolist()
    assert got.tolist()[:3] == [1234, tb + 700, 0] and got[3] >= tb and got[4] < tb


@pytest.mark.parametrize("rows,vocab,beams,k", [(16, 51865, 1, 1), (20, 51866, 5, 10), (8, 51865, 8, 16), (5, 512, 1, 1)])
def test_rule_free_entry_point_is_bit_identical(rows, vocab, beams, k):
    from mlx8_ws_audio_transformer_amd import _lib
    g = torch.Generator(device="cuda").manual_seed(rows + vocab)
    ld = vocab + (-vocab) % 128
    x = torch.randn((rows, ld), generator=g, device="cuda") * 3
    bs = torch.randn(rows, generator=g, device="cuda") if beams > 1 else None
    bits = G.banned_bits([7, 100, vocab - 3], vocab, "cuda")
    a = G.select_tokens(x, vocab, beams, bits, bs, beams > 1, k)
    L = _lib.lib()
    out = [torch.empty((rows // beams, k), dtype=dt, device="cuda") for dt in (torch.float32, torch.int64, torch.int32)]
    ws = _lib.workspace(L.awt_select_tokens_ts_workspace_bytes(rows, vocab, k), x.device)
    _lib.check(L.awt_op_select_tokens_ts(_lib.ctx(x.device), x.data_ptr(), ld, rows, vocab, beams, _lib.ptr(bits), _lib.ptr(bs), int(beams > 1), k,
                                         None, *[_lib.ptr(o) for o in out], _lib.ptr(ws), ws.numel(), _lib.stream_handle()))
    for u, v in zip(a, out):
        assert torch.equal(u, v)
