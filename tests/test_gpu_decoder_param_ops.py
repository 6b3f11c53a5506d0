"""GPU: the operators the decoder's full-parameter fine-tuning adds (include/awt.h: awt_op_embed_backward, awt_op_column_sums_ld,
awt_weight_update) against fp64, their determinism, and the in-place re-pack against freshly created handles."""
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24            # unit roundoff of fp32


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).cuda()


def _id_cases(M, L, vocab):
    g = torch.Generator().manual_seed(M)
    distinct = torch.randperm(vocab, generator=g)[:M]
    same = torch.full((M,), 7)
    repeats = torch.randint(0, 5, (M,), generator=g) * 3 + 1            # five ids: repeats inside a clip and across clips
    edges = distinct.clone(); edges[0], edges[-1], edges[M // 2] = 0, vocab - 1, 0
    low, high = repeats.clone(), repeats.clone()
    low[M // 3], high[M // 3] = -3, vocab + 4                           # out of range: the clamped row, as the forward reads it
    low[0], high[-1] = 0, vocab - 1                                     # ... shared with an in-range id of that row
    return {"distinct": distinct, "same": same, "repeats": repeats, "edges": edges, "below": low, "above": high}


@pytest.mark.parametrize("M,L,d,vocab,pos0", [(24, 12, 128, 512, 0), (7, 7, 1280, 509, 5)])
def test_embed_backward_against_fp64_index_add(M, L, d, vocab, pos0):
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    npos = pos0 + L + 3
    dx = _rand((M, d), 1)
    tok0, pos_init = _rand((vocab, d), 2), _rand((npos, d), 3)          # non-zero tables: the operator ADDS
    for name, ids in _id_cases(M, L, vocab).items():
        ids = ids.cuda()
        cl = ids.clamp(0, vocab - 1)
        runs = []
        for _ in range(2):
            dtok, dpos = tok0.clone(), pos_init.clone()
            nd.embed_backward(ids.view(M // L, L), dx, dtok, dpos, pos0)
            runs.append((dtok, dpos))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), name
        dtok, dpos = runs[0]
        # fp64 reference, and per element the sequential fp32 summation bound (n - 1) u sum|terms| plus one ulp for the add into the table
        ref = torch.zeros((vocab, d), dtype=torch.float64, device="cuda").index_add_(0, cl, dx.double())
        mag = torch.zeros((vocab, d), dtype=torch.float64, device="cuda").index_add_(0, cl, dx.double().abs())
        n = torch.zeros(vocab, dtype=torch.float64, device="cuda").index_add_(0, cl, torch.ones(M, dtype=torch.float64, device="cuda"))
        want = tok0.double() + ref
        bound = (n - 1).clamp(min=0)[:, None] * U * mag + 2 * U * want.abs()
        err = (dtok.double() - want).abs()
        print(name, "token rows: worst error / bound", float((err / bound.clamp(min=1e-30)).max()))
        assert bool((err <= bound).all()), name
        hit = n > 0
        assert torch.equal(dtok[~hit], tok0[~hit]), name                # rows no id names are not touched
        pidx = (torch.arange(M, device="cuda") % L) + pos0
        pref = torch.zeros((npos, d), dtype=torch.float64, device="cuda").index_add_(0, pidx, dx.double())
        pmag = torch.zeros((npos, d), dtype=torch.float64, device="cuda").index_add_(0, pidx, dx.double().abs())
        pwant = pos_init.double() + pref
        pbound = (M // L - 1) * U * pmag + 2 * U * pwant.abs()
        assert bool(((dpos.double() - pwant).abs() <= pbound).all()), name
        live = torch.zeros(npos, dtype=torch.bool, device="cuda"); live[pos0: pos0 + L] = True
        assert torch.equal(dpos[~live], pos_init[~live]), name


@pytest.mark.parametrize("M,ld,col,width", [(37, 3 * 128, 256, 128), (1, 3072, 0, 3072), (300, 2 * 2 * 128, 384, 128), (12, 51968, 0, 51968)])
def test_pitched_column_sums_against_fp64(M, ld, col, width):
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    a = _rand((M, ld), 4)
    win = a[:, col: col + width].double()
    ref, mag = win.sum(0), win.abs().sum(0)
    got = nd.column_sums_ld(a, col, width)
    assert torch.equal(got, nd.column_sums_ld(a, col, width))
    bound = (M - 1) * U * mag
    print("plain: worst error / bound", float(((got.double() - ref).abs() / bound.clamp(min=1e-30)).max()) if M > 1 else 0.0)
    assert bool(((got.double() - ref).abs() <= bound).all())
    init = _rand((width,), 5)
    acc = nd.column_sums_ld(a, col, width, out=init.clone(), accumulate=True)
    assert torch.equal(acc, nd.column_sums_ld(a, col, width, out=init.clone(), accumulate=True))
    want = init.double() + ref
    assert bool(((acc.double() - want).abs() <= bound + 2 * U * want.abs()).all())


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("N,K", [(1000, 768), (256, 128), (384, 3072)])
def test_weight_update_equals_a_fresh_handle(N, K, bias):
    from mlx8_ws_audio_transformer_amd.native_decoder import PackedLinear
    w0, w1 = _rand((N, K), 1, K ** -0.5), _rand((N, K), 2, K ** -0.5)
    b0, b1 = (_rand((N,), 3), _rand((N,), 4)) if bias else (None, None)
    x = _rand((40, K), 5)
    for prec in ("bf16x3", "bf16"):
        h, fresh = PackedLinear(w0, b0, prec), PackedLinear(w1, b1, prec)
        handle = h.handle
        stale = h.forward(x)
        h.update(w1, b1)
        assert h.handle == handle
        y, y_ref = h.forward(x), fresh.forward(x)
        assert torch.equal(y, y_ref) and not torch.equal(y, stale)
        dy = _rand((40, h.Np), 6)
        dy[:, N:] = 0
        assert torch.equal(h.backward_input(dy), fresh.backward_input(dy))


def test_packed_batch_update_equals_a_fresh_buffer():
    from mlx8_ws_audio_transformer_amd import native_decoder as nd
    batch, M, N, K = 3, 20, 132, 70
    a, b0, b1 = _rand((batch, M, K), 1), _rand((batch, N, K), 2), _rand((batch, N, K), 3)
    pb, fresh = nd.PackedBatch(b0), nd.PackedBatch(b1)
    buf = pb.buf.data_ptr()
    pb.update(b1)
    assert pb.buf.data_ptr() == buf
    out, ref = torch.empty((batch, M, N), device="cuda"), torch.empty((batch, M, N), device="cuda")
    nd.bmm((a, 0, K, M * K), pb, M, (out, 0, N, M * N))
    nd.bmm((a, 0, K, M * K), fresh, M, (ref, 0, N, M * N))
    assert torch.equal(out, ref)
    with pytest.raises(ValueError, match="PackedBatch.update"):
        pb.update(_rand((batch, N, K + 2), 4))


def test_weight_update_rejects_bad_arguments():
    from mlx8_ws_audio_transformer_amd import _lib
    from mlx8_ws_audio_transformer_amd.native_decoder import PackedLinear
    w = _rand((256, 128), 1)
    h = PackedLinear(w, _rand((256,), 2))
    with pytest.raises(ValueError, match=r"holds a \[256, 128\]"):         # host side, before any launch
        h.update(_rand((256, 192), 3), _rand((256,), 4))
    with pytest.raises(ValueError, match="holds a"):
        h.update(w, _rand((128,), 4))
    with pytest.raises(_lib.AwtError, match="bias"):                      # the handle has a bias: one must be given
        h.update(w, None)
    rc = _lib.lib().awt_weight_update(_lib.ctx(w.device), None, _lib.ptr(w), None, _lib.stream_handle())
    assert rc == -1 and b"weight_update" in _lib.lib().awt_last_error()   # a null handle: the library's argument error
