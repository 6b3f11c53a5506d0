"""Host checks (no GPU) of the optimizer phase: tests/adamw_reference.py against torch's own clip + AdamW in float64; the C boundary of
include/awt_optim.h; the chunk table `optim.py` builds; and the training loop of `music2midi_train.py` on torch's optimizer with a CPU stub model."""
import ctypes
import os

import pytest
import torch
from torch import nn

from mlx8_ws_audio_transformer_amd import _lib
from tests.adamw_reference import GROUP_OF, GROUPS, MAX_NORM, ReferenceAdamW, schedule_grads, schedule_params

def test_restatement_equals_torch_adamw_in_float64():
    """5 steps, two groups, lr halved after step 2, one parameter without a gradient in step 3: parameters, moments and the norm to 1e-12 relative."""
    ref = ReferenceAdamW(schedule_params(), GROUP_OF, GROUPS)
    params = [nn.Parameter(p) for p in schedule_params()]
    opt = torch.optim.AdamW([dict(params=[params[i] for i in range(4) if GROUP_OF[i] == g], **GROUPS[g]) for g in range(2)], foreach=False)
    clipped = []
    for step in range(5):
        if step == 2:
            for g, rg in zip(opt.param_groups, ref.groups):
                g["lr"] *= 0.5
                rg["lr"] *= 0.5
        grads = schedule_grads(step)
        for p, g in zip(params, grads):
            p.grad = None if g is None else g.clone()
        want_norm = torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        opt.step()
        norm, coef = ref.step(grads, MAX_NORM)
        clipped.append(float(coef) < 1.0)
        assert abs(float(norm) - float(want_norm)) <= 1e-12 * float(want_norm)
        for i, p in enumerate(params):
            st = opt.state[p]
            for got, want in ((ref.params[i], p.detach()), (ref.m[i], st["exp_avg"]), (ref.v[i], st["exp_avg_sq"])):
                assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), (step, i)
            assert ref.steps[i] == int(st["step"])
    assert ref.steps == [5, 4, 5, 5] and any(clipped) and not all(clipped)


# ------------------------------------------------------------------------------------------------ the C boundary
@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.LIB_PATH):
        from mlx8_ws_audio_transformer_amd.build import build
        build(verbose=False)
    return _lib.lib()


def test_every_declaration_of_awt_optim_h_is_exported_and_bound(built):
    names = _lib.declared_symbols(_lib.OPTIM_HEADER_PATH)
    assert names == ["awt_op_adamw_step", "awt_op_adamw_workspace_bytes", "awt_optim_chunk_elems"]
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), f"{n} declared in include/awt_optim.h but not exported by libawt.so"
        assert n in _lib._SIGNATURES, f"{n} has no ctypes signature in _lib.py"
    assert not set(names) & set(_lib.declared_symbols()), "the optimizer's declarations live in their own header, not in awt.h"
    assert len(_lib._SIGNATURES["awt_op_adamw_step"][1]) == 13


def test_chunk_and_workspace_queries_need_no_gpu(built):
    from mlx8_ws_audio_transformer_amd import optim
    C = optim.chunk_elems()
    assert C == built.awt_optim_chunk_elems() and C >= 1024 and C % 4 == 0
    assert optim.workspace_bytes(0) == 0
    one, many = optim.workspace_bytes(1), optim.workspace_bytes(1000)
    assert one >= 4 + 16 and many >= 1000 * (4 + 16) and many > one        # one fp32 partial per chunk, two fp64 bias corrections per tensor (<= chunks)
    assert one % 256 == 0 and many % 256 == 0


def test_the_chunk_table_covers_every_element_exactly_once(built):
    from mlx8_ws_audio_transformer_amd import optim
    C = optim.chunk_elems()
    for sizes in ([1, C - 1, C, C + 1], [1] * 300, [2 * C + 7, 3, C]):
        first = optim.chunk_table(sizes)
        assert len(first) == len(sizes) + 1 and first[0] == 0
        for t, n in enumerate(sizes):
            covered = [0] * n
            assert first[t + 1] > first[t], "every tensor has at least one chunk"
            for chunk in range(first[t], first[t + 1]):                    # what a workgroup does with its chunk (csrc/optim.hip)
                off = (chunk - first[t]) * C
                for e in range(off, min(off + C, n)):
                    covered[e] += 1
            assert covered == [1] * n, (sizes, t)
        assert first[-1] == sum(-(-n // C) for n in sizes)
    with pytest.raises(ValueError):
        optim.chunk_table([4, 0])
    rows = optim.tensor_table([(16, 32, 48, 64, 5, 1, 3)])
    assert rows.shape == (1, 6) and rows.dtype == torch.int64 and rows[0].tolist() == [16, 32, 48, 64, 5, 1 | (3 << 32)]
    g = optim.group_table([(1e-3, 0.5, 0.9, 0.999, 1e-8)])
    assert g.shape == (1, 8) and g.dtype == torch.float32 and g[0, 5:].tolist() == [0.0, 0.0, 0.0]


def test_fused_adamw_refuses_what_the_kernel_does_not_compute(built):
    from mlx8_ws_audio_transformer_amd import FusedAdamW
    p = nn.Parameter(torch.zeros(4))
    for kw in (dict(amsgrad=True), dict(maximize=True)):
        with pytest.raises(ValueError, match="amsgrad=False and maximize=False"):
            FusedAdamW([p], **kw)
    with pytest.raises(ValueError, match="fp32 contiguous"):
        FusedAdamW([nn.Parameter(torch.zeros(4, dtype=torch.float64))])
    with pytest.raises(ValueError, match="fp32 contiguous"):
        FusedAdamW([nn.Parameter(torch.zeros(4, 4).t()[:, :2])])
    opt = FusedAdamW([p, p], lr=1e-3)                                       # listed twice: one counter
    assert len(opt._index) == 1 and set(opt.defaults) == set(torch.optim.AdamW([p]).defaults)
    with pytest.raises(ValueError, match="closure"):
        opt.step(lambda: None)
    if not torch.cuda.is_available():
        p.grad = torch.ones(4)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            opt.step()


# ------------------------------------------------------------------------------------------------ the loop, on torch's optimizer and a CPU stub
class _Stub(nn.Module):
    """Two layers under the reference's two names; in eval mode the loss does not depend on the parameters (so the validation loss never improves)."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.cross_attention_adapter, self.text_decoder = nn.Linear(6, 6), nn.Module()
        self.text_decoder.model = nn.Module()
        self.text_decoder.model.embed_tokens = nn.Embedding(11, 6)
        self.text_decoder.model.embed_tokens.weight.requires_grad_(False)
        self.text_decoder.head = nn.Linear(6, 11)
        self.audio_encoder = nn.Linear(2, 2).requires_grad_(False)

    def forward(self, waveforms, sampling_rate, target_token_ids, attention_mask=None):
        assert len(waveforms) == target_token_ids.shape[0] and sampling_rate == 16000
        h = self.cross_attention_adapter(self.text_decoder.model.embed_tokens(target_token_ids))
        if not self.training:
            return h.sum() * 0 + 2.5
        logits = self.text_decoder.head(h)
        return nn.functional.cross_entropy(logits[:, :-1].reshape(-1, 11), target_token_ids[:, 1:].reshape(-1))


def _dataset(n):
    gen = torch.Generator().manual_seed(5)
    return [{"waveform": torch.zeros(3 + i).numpy(), "sampling_rate": 16000, "input_ids": torch.randint(0, 11, (9,), generator=gen),
             "attention_mask": torch.ones(9, dtype=torch.long), "filename": f"clip{i}.wav"} for i in range(n)]


def test_setup_optimizers_groups_by_the_references_names():
    from mlx8_ws_audio_transformer_amd import collate_fn, setup_optimizers
    model = _Stub()
    opt = setup_optimizers(model, optimizer="torch", log=lambda *_: None)
    assert isinstance(opt, torch.optim.AdamW) and [g["name"] for g in opt.param_groups] == ["adapter", "qwen"]
    assert [g["lr"] for g in opt.param_groups] == [1e-4, 2e-5] and all(g["weight_decay"] == 1e-4 for g in opt.param_groups)
    names = {id(p): n for n, p in model.named_parameters()}
    assert sorted(names[id(p)] for p in opt.param_groups[0]["params"]) == ["cross_attention_adapter.bias", "cross_attention_adapter.weight"]
    assert sorted(names[id(p)] for p in opt.param_groups[1]["params"]) == ["text_decoder.head.bias", "text_decoder.head.weight"]
    with pytest.raises(ValueError, match="fused"):
        setup_optimizers(model, optimizer="sgd")
    batch = collate_fn(_dataset(3))
    assert set(batch) == {"waveforms", "sampling_rate", "input_ids", "attention_mask", "filenames"}
    assert batch["input_ids"].shape == (3, 9) and len(batch["waveforms"]) == 3 and batch["filenames"][2] == "clip2.wav"
    with pytest.raises(AssertionError):
        collate_fn([dict(_dataset(1)[0], sampling_rate=8000), _dataset(1)[0]])


def test_checkpoint_has_the_references_keys_and_reloads(tmp_path):
    from mlx8_ws_audio_transformer_amd import load_checkpoint, save_checkpoint, train_music2midi
    from mlx8_ws_audio_transformer_amd.music2midi_train import CHECKPOINT_KEYS
    model = _Stub()
    out = train_music2midi(model, _dataset(6), _dataset(2), epochs=1, batch_size=2, optimizer="torch", models_dir=str(tmp_path), log=lambda *_: None)
    assert sorted(os.listdir(tmp_path)) == ["best_model.pt", "checkpoint_epoch_1.pt"]
    assert len(out["train_losses"]) == 1 and out["val_losses"] == [2.5] and out["best_val_loss"] == 2.5
    ck = torch.load(tmp_path / "checkpoint_epoch_1.pt", map_location="cpu")
    assert tuple(ck) == CHECKPOINT_KEYS == ("epoch", "trainable_state_dict", "critical_frozen_state_dict", "optimizer_state_dict", "loss", "config")
    trainable = {n for n, p in model.named_parameters() if p.requires_grad}
    assert set(ck["trainable_state_dict"]) == trainable and "audio_encoder.weight" not in ck["trainable_state_dict"]
    assert set(ck["critical_frozen_state_dict"]) == {"text_decoder.model.embed_tokens.weight"}
    assert ck["epoch"] == 1 and ck["loss"] == 2.5 and ck["config"]["lr_adapter"] == 1e-4 and ck["config"]["batch_size"] == 2

    other = _Stub()
    with torch.no_grad():
        for p in other.parameters():
            p.add_(1.0)
    from mlx8_ws_audio_transformer_amd import setup_optimizers
    opt = setup_optimizers(other, optimizer="torch", log=lambda *_: None)
    assert load_checkpoint(other, opt, str(tmp_path / "best_model.pt")) == (1, 2.5)
    for (n, p), (_, q) in zip(model.named_parameters(), other.named_parameters()):
        if n in trainable or "embed_tokens" in n:
            assert torch.equal(p, q), n
        else:
            assert not torch.equal(p, q), n                                 # the frozen tower is not in the file
    want = out["optimizer"].state_dict()["state"]
    got = opt.state_dict()["state"]
    assert want.keys() == got.keys() and all(torch.equal(want[k]["exp_avg"], got[k]["exp_avg"]) and float(want[k]["step"]) == float(got[k]["step"]) == 3.0 for k in want)
    path = save_checkpoint(other, opt, 7, 0.25, str(tmp_path))
    assert os.path.basename(path) == "checkpoint_epoch_7.pt" and "best_model.pt" in os.listdir(tmp_path)


def test_learning_rates_halve_after_three_epochs_without_improvement():
    """ReduceLROnPlateau(factor=0.5, patience=2): the stub's validation loss is constant, so epoch 1 sets the best and epochs 2, 3, 4 do not improve
    on it: the third of them halves both groups' rates, not the second."""
    from mlx8_ws_audio_transformer_amd import train_music2midi
    out = train_music2midi(_Stub(), _dataset(4), _dataset(2), epochs=5, batch_size=2, optimizer="torch", log=lambda *_: None)
    assert out["val_losses"] == [2.5] * 5
    assert out["lrs"] == [[1e-4, 2e-5]] * 3 + [[5e-5, 1e-5]] * 2
    assert len(out["train_losses"]) == 5 and out["train_losses"][-1] < out["train_losses"][0]
    without = train_music2midi(_Stub(), _dataset(4), None, epochs=2, batch_size=2, optimizer="torch", log=lambda *_: None)
    assert without["val_losses"] == [] and len(without["train_losses"]) == 2 and without["lrs"] == [[1e-4, 2e-5]] * 2
