"""GPU: full-parameter fine-tuning of the encoder (`train_encoder=True`, the reference's fineTune.py semantics on the encoder) through the
fineTune.py call surface: the loss falls and only the encoder moves, the updated weights reach the library, gradient accumulation and
sharding agree with the full batch, the checkpoint directory round-trips, `WhisperAudioEncoder(freeze_encoder=False)` trains, and two
ranks exchange the flat gradient buffer."""
import os
import socket

import numpy as np
import pytest
import torch

from mlx8_ws_audio_transformer_amd import weights as wts
from oracle import encoder as oracle_enc
from oracle import logmel as oracle_mel
from tests.util import piano_clips_f32

pytestmark = pytest.mark.gpu

FROZEN = "embed_positions.weight"


def _batch(cfg, B, first=0):
    mel = oracle_mel.whisper_logmel(piano_clips_f32(B, first), n_samples=cfg.n_frames * 160)
    g = torch.Generator().manual_seed(first)
    labels = torch.randint(3, 1000, (B, 6), generator=g)
    labels[:, 0] = 50258                  # every row has six label tokens: shard / micro-batch loss means weigh equally
    return {"input_features": torch.from_numpy(mel), "labels": labels}


def _model(cfg, **kw):
    from mlx8_ws_audio_transformer_amd.finetune import WhisperLoRAModel
    return WhisperLoRAModel(cfg, None, train_encoder=True, decoder_layers=1, **kw)


def _trainer(cfg, **args):
    from mlx8_ws_audio_transformer_amd.finetune import Seq2SeqTrainer, Seq2SeqTrainingArguments
    model = _model(cfg)
    a = dict(learning_rate=0.0, warmup_steps=0, max_steps=4, max_grad_norm=0.0, predict_with_generate=False)     # lr 0: the step leaves the gradients to look at
    a.update(args)
    return model, Seq2SeqTrainer(args=Seq2SeqTrainingArguments(**a), model=model)


def test_loss_decreases_only_the_encoder_moves_and_the_library_sees_the_update(tmp_path):
    from mlx8_ws_audio_transformer_amd.collator import DataCollatorSpeechSeq2SeqWithPadding
    from mlx8_ws_audio_transformer_amd.finetune import Seq2SeqTrainer, Seq2SeqTrainingArguments
    cfg = wts.config("mini", True)
    model = _model(cfg)
    assert model.lora_parameters() == [] and len(model.trainable_parameters()) == len(list(model.encoder.parameters())) - 1
    enc0 = {k: v.detach().clone() for k, v in model.encoder.state_dict().items()}
    dec0 = {k: v.detach().clone() for k, v in model.decoder.state_dict().items()}
    b = _batch(cfg, 4)
    ds = [{"input_features": b["input_features"][i].numpy(), "labels": b["labels"][i].tolist()} for i in range(4)]
    args = Seq2SeqTrainingArguments(output_dir=str(tmp_path), per_device_train_batch_size=4, learning_rate=5e-4, warmup_steps=1,
                                    max_steps=20, logging_steps=1, save_steps=20, predict_with_generate=False)
    tr = Seq2SeqTrainer(args=args, model=model, train_dataset=ds, eval_dataset=ds,
                        data_collator=DataCollatorSpeechSeq2SeqWithPadding(processor=None, decoder_start_token_id=50258), tokenizer=None)
    assert tr.bucket.numel == sum(p.numel() for n, p in model.encoder.named_parameters() if n != FROZEN)
    tr.train()
    losses = [h["loss"] for h in tr.log_history if "loss" in h]
    print("losses", [round(l, 4) for l in losses])
    assert losses[-1] < losses[0] - 0.05, losses
    enc1 = model.encoder.state_dict()
    for k, v in enc0.items():
        assert torch.equal(enc1[k], v) == (k == FROZEN), k            # every encoder parameter moved, the position table did not
    for k, v in model.decoder.state_dict().items():
        assert torch.equal(v, dec0[k]), k                              # the decoder's base weights stay frozen
    # the library runs on the UPDATED weights: the native forward equals the oracle forward on them
    mel = b["input_features"][:2]
    ref = oracle_enc.encoder_forward({k: v.detach().cpu().numpy() for k, v in enc1.items()}, mel.numpy(), cfg.heads).numpy()
    with torch.no_grad():
        got = model.encoder(mel.cuda()).last_hidden_state.cpu().numpy()
    stale = oracle_enc.encoder_forward({k: v.cpu().numpy() for k, v in enc0.items()}, mel.numpy(), cfg.heads).numpy()
    assert float(np.abs(ref - stale).max()) > 1e-2                     # the update is visible at this tolerance
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-3)
    # save_steps = 20: the checkpoint of this mode is the full directory, not an adapter file
    assert not (tmp_path / "lora_adapters.pt").exists() and (tmp_path / "config.json").exists()


def test_two_micro_batches_equal_one_batch():
    cfg = wts.config("mini", True)
    b = _batch(cfg, 4)
    flats = {}
    for ga in (1, 2):
        model, tr = _trainer(cfg)
        tr.training_step(b if ga == 1 else [{k: v[:2] for k, v in b.items()}, {k: v[2:] for k, v in b.items()}])
        flats[ga] = tr.bucket.flat.clone()
    assert float(flats[1].abs().max()) > 0
    assert float((flats[1] - flats[2]).abs().max()) < 2e-3 * float(flats[1].abs().max())


def test_sharded_gradients_average_to_full_batch_gradient():
    cfg = wts.config("mini", True)
    model = _model(cfg)
    full = _batch(cfg, 4)

    def grads(batch):
        model.zero_grad()
        model(input_features=batch["input_features"].cuda(), labels=batch["labels"].cuda()).loss.backward()
        return torch.cat([p.grad.flatten() for p in model.trainable_parameters()]).clone()

    g_full = grads(full)
    halves = [{k: v[i:i + 2] for k, v in full.items()} for i in (0, 2)]
    g_avg = (grads(halves[0]) + grads(halves[1])) / 2
    rel = (g_full - g_avg).abs().max() / g_full.abs().max()
    assert rel < 1e-3, float(rel)


def test_checkpoint_directory_roundtrips_the_trained_weights(tmp_path):
    from mlx8_ws_audio_transformer_amd.finetune import WhisperLoRAModel
    cfg = wts.config("mini", True)
    model, tr = _trainer(cfg, learning_rate=1e-3)
    tr.training_step(_batch(cfg, 2))
    path = tr.save_model(str(tmp_path / "whisper-mini-full"))
    assert not os.path.exists(os.path.join(path, "lora_adapters.pt"))
    again = WhisperLoRAModel.from_pretrained(path, train_encoder=True)
    assert again.encoder.train_base and again.encoder.precision == "bf16x3"
    a, b = model.encoder.state_dict(), again.encoder.state_dict()
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for k, v in model.decoder.state_dict().items():
        assert torch.equal(v, again.decoder.state_dict()[k]), k
    assert [n for n, p in again.encoder.named_parameters() if not p.requires_grad] == [FROZEN]


def test_audio_encoder_with_an_unfrozen_encoder_trains():
    from mlx8_ws_audio_transformer_amd import synth
    from mlx8_ws_audio_transformer_amd.audio_encoder import WhisperAudioEncoder
    cfg = wts.config("mini", False)
    pcm = torch.from_numpy(np.stack([synth.pcm_i16_to_f32(c) for c in synth.synth_clips_i16(2, seed=1234, first=0)]))
    tower = WhisperAudioEncoder(cfg, freeze_encoder=False)
    out = tower(pcm, 16000)
    assert out.requires_grad and out.shape == (2, 1500, cfg.d_model)
    out.square().mean().backward()
    for n, p in tower.encoder.named_parameters():
        assert (p.grad is None) == (n == FROZEN), n
        assert n == FROZEN or float(p.grad.abs().max()) > 0, n
    with torch.no_grad():
        assert not tower(pcm, 16000).requires_grad
    frozen = WhisperAudioEncoder(cfg, freeze_encoder=True, precision="bf16x3")
    frozen.encoder.load_state_dict(tower.encoder.state_dict())
    ref = frozen(pcm, 16000)
    assert not ref.requires_grad
    assert float((ref - out.detach()).abs().max()) < 1e-3             # the two paths (one fused call, log-mel then training forward) agree


def _rank_main(rank, world, port, path):
    import torch.distributed as dist
    from mlx8_ws_audio_transformer_amd.dist import shard_range
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = wts.config("mini", True)
    full = _batch(cfg, 4, 40)
    lo, hi = shard_range(4, rank, world)
    model, tr = _trainer(cfg)
    assert "gloo" in tr.exchange and tr.comm is None
    tr.training_step({k: v[lo:hi] for k, v in full.items()})
    torch.save({"flat": tr.bucket.flat.cpu(), "checksums": tr.exchange_checksums()}, os.path.join(path, f"rank{rank}.pt"))
    dist.destroy_process_group()


def test_two_gloo_ranks_exchange_the_base_gradients(tmp_path):
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    [p.start() for p in procs]
    [p.join(600) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    r0, r1 = (torch.load(tmp_path / f"rank{r}.pt") for r in range(2))
    assert r0["checksums"][0] == r0["checksums"][1] == r1["checksums"][0] == r1["checksums"][1]      # the same buffer on both ranks after the exchange
    assert torch.equal(r0["flat"], r1["flat"])
    cfg = wts.config("mini", True)
    model, tr = _trainer(cfg)
    assert tr.exchange == "none"
    tr.training_step(_batch(cfg, 4, 40))
    want = tr.bucket.flat.cpu()
    rel = float((r0["flat"] - want).abs().max() / want.abs().max())
    assert rel < 1e-3, rel


def test_in_backward_exchange_covers_the_base_gradients():
    """AWT_BWD_ALLREDUCE on a one-rank communicator: the layer groups and, last, the lowest group with the conv stem and the final
    LayerNorm in front of it go through the side-stream exchange; averaging over one rank is the identity."""
    cfg = wts.config("mini", True)
    full = _batch(cfg, 4, 40)
    micro = [{k: v[:2] for k, v in full.items()}, {k: v[2:] for k, v in full.items()}]
    out = {}
    for native in (False, True):
        model, tr = _trainer(cfg)
        if native:
            tr._setup_exchange(force_native=True)
            assert tr.comm is not None and "rccl" in tr.exchange
        losses = [tr.training_step(full)]
        first = tr.bucket.flat.clone()
        losses.append(tr.training_step(micro))
        torch.cuda.synchronize()
        out[native] = (losses, first, tr.bucket.flat.clone())
    assert out[True][0] == out[False][0]
    assert torch.equal(out[True][1], out[False][1]) and torch.equal(out[True][2], out[False][2])
