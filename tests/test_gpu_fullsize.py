"""GPU: BASELINE.json's full-size workload (Whisper-small, parity mode, 64 clips) checked through size-independent
properties -- the oracle needs ~1 s per clip at this size, so only a sample of clips is compared against it."""
import numpy as np
import pytest
import torch

from mlx8_ws_audio_transformer_amd import synth, weights as wts
from oracle import encoder as oracle_enc
from oracle import logmel as oracle_mel
from tests.util import tuning

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["f16f8", "bf16x3"])      # the headline mode and the split-bf16 mode the training path uses
def full(request):
    from mlx8_ws_audio_transformer_amd.encoder import NativeWhisperEncoder
    cfg = wts.config("small")
    pcm = torch.from_numpy(synth.synth_clips_i16(64, seed=1234, first=100)).cuda()
    enc = NativeWhisperEncoder(cfg, precision=request.param, seed=0, init_profile="hf").eval()
    hidden, feats = enc.encode_pcm(pcm, return_features=True)
    return cfg, pcm, enc, hidden, feats


def test_rows_are_layernormed_and_finite(full):
    cfg, pcm, enc, hidden, feats = full
    assert tuple(hidden.shape) == (64, 1500, 768) and torch.isfinite(hidden).all()
    # final LayerNorm with gamma 1 / beta 0: every row has mean 0 and variance 1
    assert hidden.mean(-1).abs().max().item() < 1e-4
    assert (hidden.var(-1, unbiased=False) - 1).abs().max().item() < 1e-3
    # log-mel: padding frames are one constant per clip, clip maximum minus 2.0 after the (x + 4) / 4 rescale
    assert torch.equal(feats[:, :, 402:], feats[:, :1, 402:403].expand(-1, 80, 2598))
    assert (feats.amax(dim=(1, 2)) - 2.0 - feats[:, 0, 402]).abs().max().item() < 1e-6


def test_batch_permutation_and_chunking_are_exact(full):
    cfg, pcm, enc, hidden, feats = full
    from mlx8_ws_audio_transformer_amd.encoder import NativeWhisperEncoder
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(5)).cuda()
    assert torch.equal(enc.encode_pcm(pcm[perm].contiguous()), hidden[perm])        # clips are independent
    small_chunks = NativeWhisperEncoder(cfg, precision=enc.precision, seed=0, init_profile="hf", chunk_clips=24).eval()
    assert torch.equal(small_chunks.encode_pcm(pcm), hidden)                            # chunk size is invisible


def test_ping_pong_mlp_route_is_bit_identical_to_the_128_row_tiles(full):
    # at this size the f16f8 mode takes the persistent ping-pong GEMM for fc1 / fc2 ("gemm_pp" = 1, automatic): the same products in the same order as the
    # 128 x 256 kernel's 16 x 16 form, so switching it off -- or on for all four projections -- must not change one bit of the hidden states
    cfg, pcm, enc, hidden, feats = full
    if enc.precision != "f16f8":
        pytest.skip("the ping-pong GEMM is an f16f8 kernel")
    with tuning(gemm_pp=0):
        off = enc.encode_pcm(pcm)
    with tuning(gemm_pp=2, gemm_pp_mask=15):
        every = enc.encode_pcm(pcm)
    assert torch.equal(off, hidden) and torch.equal(every, hidden)


def test_duplicate_and_silent_clips(full):
    cfg, pcm, enc, hidden, feats = full
    p2 = pcm.clone()
    p2[7] = p2[3]
    p2[11] = 0
    h2, f2 = enc.encode_pcm(p2, return_features=True)
    assert torch.equal(h2[7], h2[3]) and torch.equal(h2[3], hidden[3])
    assert torch.all(f2[11] == -1.5)                                                    # (log10(1e-10) + 4) / 4
    assert torch.isfinite(h2[11]).all()


def test_sampled_clips_match_oracle(full):
    cfg, pcm, enc, hidden, feats = full
    idx = [0, 31, 63]
    clips = [synth.pcm_i16_to_f32(pcm[i].cpu().numpy()) for i in idx]
    mel = oracle_mel.whisper_logmel(clips)
    np.testing.assert_allclose(feats[idx].cpu().numpy(), mel, rtol=0, atol=1e-5)
    ref = oracle_enc.encoder_forward(wts.init_encoder_weights(cfg, 0, "hf"), mel, cfg.heads).numpy()
    assert np.abs(hidden[idx].cpu().numpy() - ref).max() < 1e-3


# ---------------------------------------------------------------- BASELINE.json configs[2]: LoRA r = 8 fine-tune step, B = 64
@pytest.fixture(scope="module")
def step64():
    from mlx8_ws_audio_transformer_amd.feature_extraction import logmel_whisper_device
    from mlx8_ws_audio_transformer_amd.finetune import WhisperLoRAModel
    cfg = wts.config("small")
    pcm = torch.from_numpy(synth.synth_clips_i16(64, seed=1234, first=200)).cuda()
    feats = logmel_whisper_device(pcm, n_frames=cfg.n_frames)
    g = torch.Generator().manual_seed(0)
    labels = torch.randint(0, 51864, (64, 12), generator=g); labels[:, 0] = 50258

    def make():
        model = WhisperLoRAModel(cfg, wts.LoraSpec(r=8, alpha=16.0), seed=0)
        with torch.no_grad():
            for p in model.lora_parameters():      # non-zero B so that both adapter matrices receive gradient
                if p.shape[1] == 8:
                    p.copy_(torch.from_numpy((0.02 * wts.unit_variates("b64", p.numel(), 1)).reshape(p.shape).astype(np.float32)))
        return model
    return cfg, feats, labels.cuda(), make


def test_b64_encoder_backward_is_bit_reproducible_and_batch_mean_decomposes(step64):
    cfg, feats, labels, make = step64
    model = make()

    def grads(sl):
        model.zero_grad()
        model(input_features=feats[sl], labels=labels[sl]).loss.backward()
        return torch.cat([p.grad.flatten() for p in model.encoder.lora_parameters_library_order()]).clone()

    g_full = grads(slice(0, 64))
    assert torch.isfinite(g_full).all() and float(g_full.abs().max()) > 0
    # every row carries 12 label tokens, so the batch-mean loss is the mean of the two half-batch means
    g_half = (grads(slice(0, 32)) + grads(slice(32, 64))) / 2
    assert float((g_full - g_half).abs().max()) < 1e-3 * float(g_full.abs().max())
    # the native backward has no atomics: a fixed upstream gradient gives bit-identical adapter gradients at B = 64
    dout = torch.from_numpy((wts.unit_variates("dout64", 64 * 1500 * 768, 7) / 40.0).astype(np.float32)).cuda().view(64, 1500, 768)
    runs = []
    for _ in range(2):
        model.zero_grad()
        model.encoder(feats).last_hidden_state.backward(dout)
        runs.append(torch.cat([p.grad.flatten() for p in model.encoder.lora_parameters_library_order()]).clone())
    assert torch.equal(runs[0], runs[1])


def test_b64_training_steps_reduce_the_loss(step64):
    from mlx8_ws_audio_transformer_amd.finetune import Seq2SeqTrainer, Seq2SeqTrainingArguments
    cfg, feats, labels, make = step64
    model = make()
    args = Seq2SeqTrainingArguments(per_device_train_batch_size=64, learning_rate=1e-3, warmup_steps=0, max_steps=10, predict_with_generate=False)
    tr = Seq2SeqTrainer(args=args, model=model)
    assert tr.bucket.numel == 12 * 2 * 2 * 8 * 768                  # r = 8 on q_proj, v_proj of 12 layers: A and B
    flat_ptr = tr.bucket.flat.data_ptr()
    before = torch.cat([p.detach().flatten().clone() for p in model.lora_parameters()])
    losses = [tr.training_step({"input_features": feats, "labels": labels}) for _ in range(3)]
    assert all(np.isfinite(l) for l in losses)
    assert losses[1] < losses[0] and losses[2] < losses[1], losses
    after = torch.cat([p.detach().flatten() for p in model.lora_parameters()])
    assert float((after - before).abs().max()) > 0
    # the gradients never left the flat buffer: every adapter .grad is still a view of it
    assert tr.bucket.flat.data_ptr() == flat_ptr and tr.bucket.bind(keep=True) == 0
    assert model.encoder.lora_parameters_library_order()[0].grad.data_ptr() == flat_ptr


# ---------------------------------------------------------------- BASELINE.json configs[3], one rank's share: LoRA r = 16, 64 clips per GPU (global batch 512 over 8 GPUs)
def test_r16_b64_per_rank_step_of_the_dp8_configuration():
    """What ONE rank of configs[3] runs: r = 16 adapters on q_proj / v_proj (589 824 gradient elements = 2.36 MB, the buffer the 8-GPU run all-reduces),
    64 clips.  On this one GPU the exchange goes through libawt's RCCL communicator with a single rank (ncclAvg over one rank = identity), issued
    inside the backward on the side stream: the step must fit in memory, time its two bucket reductions, leave the flat buffer bit-identical to a
    run without the communicator, and be bit-reproducible."""
    from mlx8_ws_audio_transformer_amd.feature_extraction import logmel_whisper_device
    from mlx8_ws_audio_transformer_amd.finetune import Seq2SeqTrainer, Seq2SeqTrainingArguments, WhisperLoRAModel
    cfg = wts.config("small")
    pcm = torch.from_numpy(synth.synth_clips_i16(64, seed=1234, first=300)).cuda()
    feats = logmel_whisper_device(pcm, n_frames=cfg.n_frames)
    g = torch.Generator().manual_seed(1)
    labels = torch.randint(0, 51864, (64, 12), generator=g); labels[:, 0] = 50258
    labels = labels.cuda()

    def run(native_comm):
        torch.manual_seed(0)
        model = WhisperLoRAModel(cfg, wts.LoraSpec(r=16, alpha=16.0), seed=0)
        with torch.no_grad():
            for p in model.lora_parameters():      # non-zero B so that both adapter matrices receive gradient
                if p.shape[1] == 16:
                    p.copy_(torch.from_numpy((0.02 * wts.unit_variates("r16", p.numel(), 1)).reshape(p.shape).astype(np.float32)))
        args = Seq2SeqTrainingArguments(per_device_train_batch_size=64, learning_rate=1e-4, warmup_steps=0, max_steps=10, predict_with_generate=False)
        tr = Seq2SeqTrainer(args=args, model=model)
        if native_comm:
            tr._setup_exchange(force_native=True)
        assert tr.bucket.numel == 12 * 2 * 2 * 16 * 768 == 589824
        rep0 = tr.exchange_report()
        loss = tr.training_step({"input_features": feats, "labels": labels})
        rep = tr.exchange_report()
        flat = tr.bucket.flat.detach().clone()
        sums = tr.exchange_checksums()
        peak = torch.cuda.max_memory_allocated() / 2 ** 30
        del tr, model
        torch.cuda.empty_cache()
        return loss, flat, rep0, rep, sums, peak

    loss_a, flat_a, _, rep_plain, _, _ = run(False)
    loss_b, flat_b, rep0, rep, sums, peak = run(True)
    loss_c, flat_c, _, _, sums_c, _ = run(True)
    print("r16 B64 step: loss %.5f, peak device memory %.1f GiB, exchange %s" % (loss_b, peak, rep))
    assert np.isfinite(loss_b) and torch.isfinite(flat_b).all() and float(flat_b.abs().max()) > 0
    assert rep_plain["rccl_ranks"] == 0 and rep["rccl_ranks"] == 1 and rep["flat_grad_elems"] == 589824
    assert rep0.get("buckets") == [] and len(rep["buckets"]) == 2                      # two layer groups, each timed on the side stream
    assert sum(b["bytes"] for b in rep["buckets"]) == 589824 * 4 and all(b["ms"] >= 0 for b in rep["buckets"])
    assert torch.equal(flat_a, flat_b) and loss_a == loss_b                            # a one-rank ncclAvg is the identity
    assert torch.equal(flat_b, flat_c) and sums == sums_c                              # bit-reproducible, checksum included
    assert peak < 200.0
