"""The reference's music2midi training loop (.charles/music2midi/train.py) on `MusicTranscriptionModel`: two parameter groups (the adapter at 1e-4, Qwen at
2e-5), AdamW with weight decay 1e-4, global-norm clipping at 1.0, `ReduceLROnPlateau(factor=0.5, patience=2)` on the validation loss, best-model
tracking and checkpoints that hold only the trainable state.  The optimizer phase runs on `optim.FusedAdamW` (`optimizer="fused"`, the default: clip and
step are one operator call) or on torch's own (`optimizer="torch"`: `clip_grad_norm_` + `torch.optim.AdamW`, the reference's two calls).

What the reference file also does and this module leaves out: wandb logging, the tqdm progress bar, the colour logger (progress goes to the `log`
callable, `print` by default), loading the tokenizer, `MusicDataset` and the random train / validation split -- `train_music2midi` takes any dataset of
{"waveform", "sampling_rate", "input_ids", "attention_mask", "filename"} items -- and the parameter-count report.

Two deliberate differences.  The loop adds the batch losses on the device and reads the sum once per epoch where the reference reads every batch's loss
(`loss.item()`); the mean is the same sum.  `save_checkpoint` stores the requires_grad parameters under `trainable_state_dict`, which is what the
reference's comment says and what its identity test against `state_dict()`'s detached tensors does not select.
"""
from __future__ import annotations

import os
from typing import Callable, Dict, List, Optional

import torch
from torch.utils.data import DataLoader

from .optim import FusedAdamW

LR_ADAPTER, LR_QWEN, WEIGHT_DECAY, GRAD_CLIP_NORM = 1e-4, 2e-5, 1e-4, 1.0          # train.py:52-55
CHECKPOINT_KEYS = ("epoch", "trainable_state_dict", "critical_frozen_state_dict", "optimizer_state_dict", "loss", "config")


def collate_fn(batch: List[Dict]) -> Dict:
    """train.py:207-228: the waveforms stay a list (their lengths differ), ids and masks are stacked, one sampling rate per batch."""
    rates = {item["sampling_rate"] for item in batch}
    assert len(rates) == 1, "All samples must have same sampling rate"
    return {"waveforms": [item["waveform"] for item in batch], "sampling_rate": batch[0]["sampling_rate"],
            "input_ids": torch.stack([item["input_ids"] for item in batch]), "attention_mask": torch.stack([item["attention_mask"] for item in batch]),
            "filenames": [item["filename"] for item in batch]}


def setup_optimizers(model, lr_adapter: float = LR_ADAPTER, lr_qwen: float = LR_QWEN, weight_decay: float = WEIGHT_DECAY, optimizer: str = "fused",
                     log: Callable = print):
    """train.py:230-279: every requires_grad parameter whose name holds `cross_attention_adapter` goes to the group named "adapter", `text_decoder` to
    "qwen", anything else to "adapter" with a warning; AdamW over the two groups.  optimizer: "fused" (`FusedAdamW`) or "torch" (`torch.optim.AdamW`)."""
    if optimizer not in ("fused", "torch"):
        raise ValueError(f"optimizer must be 'fused' or 'torch', got {optimizer!r}")
    adapter, qwen = [], []
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        if "audio_encoder" in name:
            log(f"warning: the audio tower's parameter {name} is trainable")
        if "cross_attention_adapter" in name:
            adapter.append(p)
        elif "text_decoder" in name:
            qwen.append(p)
        else:
            log(f"warning: unknown trainable parameter {name}: put into the adapter group")
            adapter.append(p)
    groups = [{"params": adapter, "lr": lr_adapter, "name": "adapter"}, {"params": qwen, "lr": lr_qwen, "name": "qwen"}]
    log(f"adapter parameters: {sum(p.numel() for p in adapter):,}; qwen parameters: {sum(p.numel() for p in qwen):,}")
    return (FusedAdamW if optimizer == "fused" else torch.optim.AdamW)(groups, weight_decay=weight_decay)


def _model_device(model) -> torch.device:
    return next(model.parameters()).device


def _loss_of(model, batch, device) -> torch.Tensor:
    return model(batch["waveforms"], batch["sampling_rate"], batch["input_ids"].to(device), batch["attention_mask"].to(device))


def validate_model(model, val_loader, device=None) -> float:
    """train.py:364-385: the mean loss over the loader in eval mode without gradients (inf for an empty loader); one host read."""
    device = device or _model_device(model)
    model.eval()
    total, n = None, 0
    with torch.no_grad():
        for batch in val_loader:
            loss = _loss_of(model, batch, device).detach()
            total = loss if total is None else total + loss
            n += 1
    return float(total) / n if n else float("inf")


def _trainable_state(model) -> dict:
    if hasattr(model, "trainable_state_dict"):
        return model.trainable_state_dict()
    return {n: p.detach() for n, p in model.named_parameters() if p.requires_grad}


def save_checkpoint(model, optimizer, epoch: int, loss: float, models_dir: str, is_best: bool = False, config: Optional[dict] = None) -> str:
    """train.py:281-334: `checkpoint_epoch_N.pt` (and `best_model.pt` when is_best) under models_dir with the reference's keys: the trainable
    parameters, the embedding / head entries whether trained or not, the optimizer's state, the loss, a config dict.  The frozen audio tower and
    the frozen decoder layers are not stored."""
    os.makedirs(models_dir, exist_ok=True)
    critical = {n: t for n, t in model.state_dict().items() if "text_decoder.model.embed_tokens" in n or "text_decoder.lm_head" in n}
    dec_cfg = getattr(getattr(model, "text_decoder", None), "config", None)
    cfg = {"vocab_size": getattr(dec_cfg, "vocab_size", None), "top_k_layers": getattr(getattr(model, "text_decoder", None), "trainable_layers", None),
           "note": "the frozen audio tower and decoder layers are not stored: they are loaded from the base models"}
    cfg.update(config or {})
    checkpoint = {"epoch": epoch, "trainable_state_dict": _trainable_state(model), "critical_frozen_state_dict": critical,
                  "optimizer_state_dict": optimizer.state_dict(), "loss": loss, "config": cfg}
    path = os.path.join(models_dir, f"checkpoint_epoch_{epoch}.pt")
    torch.save(checkpoint, path)
    if is_best:
        torch.save(checkpoint, os.path.join(models_dir, "best_model.pt"))
    return path


def load_checkpoint(model, optimizer, checkpoint_path: str):
    """train.py:336-362: the trainable and the embedding / head entries through `load_state_dict(strict=False)`, then the optimizer's state when an
    optimizer is given; returns (epoch, loss).  A checkpoint of the older format (`model_state_dict`) loads too."""
    checkpoint = torch.load(checkpoint_path, map_location="cpu")
    if "trainable_state_dict" in checkpoint:
        model.load_state_dict(checkpoint["trainable_state_dict"], strict=False)
        if "critical_frozen_state_dict" in checkpoint:
            model.load_state_dict(checkpoint["critical_frozen_state_dict"], strict=False)
    else:
        model.load_state_dict(checkpoint["model_state_dict"], strict=False)
    if optimizer is not None and "optimizer_state_dict" in checkpoint:
        optimizer.load_state_dict(checkpoint["optimizer_state_dict"])
    return checkpoint.get("epoch", 0), checkpoint.get("loss", float("inf"))


def train_step(model, optimizer, batch, grad_clip_norm: float = GRAD_CLIP_NORM, device=None) -> torch.Tensor:
    """train.py:481-501 for one batch: zero_grad, loss, backward, clip, step.  Returns the detached loss, still on the device."""
    device = device or _model_device(model)
    optimizer.zero_grad()
    loss = _loss_of(model, batch, device)
    loss.backward()
    if isinstance(optimizer, FusedAdamW):
        optimizer.step(max_norm=grad_clip_norm)
    else:
        torch.nn.utils.clip_grad_norm_(model.parameters(), grad_clip_norm)
        optimizer.step()
    return loss.detach()


def train_music2midi(model, train_dataset, val_dataset=None, *, epochs: int = 3, batch_size: int = 4, lr_adapter: float = LR_ADAPTER,
                     lr_qwen: float = LR_QWEN, weight_decay: float = WEIGHT_DECAY, grad_clip_norm: float = GRAD_CLIP_NORM, optimizer="fused",
                     save_every_n_epochs: int = 1, models_dir: Optional[str] = None, seed: int = 42, shuffle: bool = True, log: Callable = print) -> dict:
    """train.py:387-552 (`main`) from the model on: the two-group AdamW of `setup_optimizers` (or a ready optimizer passed as `optimizer`), shuffled
    batches of `batch_size` (seeded by `seed`), per batch `train_step`; per epoch the validation loss, `ReduceLROnPlateau(mode="min", factor=0.5,
    patience=2)` on it, best-model tracking, and a checkpoint every `save_every_n_epochs` epochs or at a new best (without a validation set: the
    periodic checkpoints only, with the training loss).  models_dir=None writes no checkpoint.
    Returns {"train_losses", "val_losses" (empty without a validation set), "lrs" (per epoch, one per group, after the scheduler), "best_val_loss",
    "optimizer"}."""
    device = _model_device(model)
    opt = setup_optimizers(model, lr_adapter, lr_qwen, weight_decay, optimizer, log=log) if isinstance(optimizer, str) else optimizer
    gen = torch.Generator()
    gen.manual_seed(seed)
    train_loader = DataLoader(train_dataset, batch_size=batch_size, shuffle=shuffle, collate_fn=collate_fn, generator=gen if shuffle else None)
    val_loader = DataLoader(val_dataset, batch_size=batch_size, shuffle=False, collate_fn=collate_fn) if val_dataset is not None and len(val_dataset) else None
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=2)
    config = {"lr_adapter": lr_adapter, "lr_qwen": lr_qwen, "batch_size": batch_size}
    out = {"train_losses": [], "val_losses": [], "lrs": [], "best_val_loss": float("inf"), "optimizer": opt}
    for epoch in range(1, epochs + 1):
        model.train()
        total, n = None, 0
        for batch in train_loader:
            loss = train_step(model, opt, batch, grad_clip_norm, device)
            total = loss if total is None else total + loss           # stays on the device
            n += 1
        train_loss = float(total) / n if n else float("nan")          # the epoch's one host read
        out["train_losses"].append(train_loss)
        if val_loader is not None:
            val_loss = validate_model(model, val_loader, device)
            scheduler.step(val_loss)
            out["val_losses"].append(val_loss)
            log(f"epoch {epoch} - train loss {train_loss:.4f}, val loss {val_loss:.4f}")
            is_best = val_loss < out["best_val_loss"]
            if is_best:
                out["best_val_loss"] = val_loss
            if models_dir is not None and (epoch % save_every_n_epochs == 0 or is_best):
                save_checkpoint(model, opt, epoch, val_loss, models_dir, is_best, config)
        else:
            log(f"epoch {epoch} - train loss {train_loss:.4f}")
            if models_dir is not None and epoch % save_every_n_epochs == 0:
                save_checkpoint(model, opt, epoch, train_loss, models_dir, False, config)
        out["lrs"].append([g["lr"] for g in opt.param_groups])
    return out
