"""CPU: the host side of timestamp / long-form generate -- segment splitting and seek advance (HF `_retrieve_segment`), output padding
(`_pad_to_max_length`), the batch bookkeeping, and argument refusals that need no GPU."""
import numpy as np
import pytest
import torch

from mlx8_ws_audio_transformer_amd import generation as G
from tests.util import golden

TB = 411                     # the fixture's timestamp_begin (tools/make_golden_timestamps.py)


def _t(*x):
    return torch.tensor(x, dtype=torch.int64)


def test_double_timestamps_split_and_seek_to_the_last_one():
    seq = _t(TB + 0, 5, 6, TB + 50, TB + 50, 7, TB + 80, TB + 80, 9, 9)       # unfinished tail after the last pair
    segs, offset = G.retrieve_segment(seq, 10.0, TB, 3000, 3)
    assert [s["tokens"].tolist() for s in segs] == [[TB, 5, 6, TB + 50], [TB + 50, 7, TB + 80, TB + 80]]
    assert [s["idxs"] for s in segs] == [(3, 7), (7, 11)]
    assert segs[0]["start"] == 10.0 and segs[0]["end"] == 10.0 + 50 * 0.02
    assert segs[1]["start"] == 10.0 + 50 * 0.02 and segs[1]["end"] == 10.0 + 80 * 0.02
    assert offset == 80 * 2


def test_single_timestamp_ending_seeks_the_whole_window():
    seq = _t(TB + 0, 5, TB + 40, TB + 40, 7, TB + 90)
    segs, offset = G.retrieve_segment(seq, 0.0, TB, 2500, 3)
    assert [s["tokens"].tolist() for s in segs] == [[TB, 5, TB + 40], [TB + 40, 7, TB + 90]]
    assert segs[-1]["end"] == 90 * 0.02 and offset == 2500


def test_no_timestamps_and_lone_final_timestamp():
    segs, offset = G.retrieve_segment(_t(5, 6, 7), 30.0, TB, 1234, 3)        # no timestamp: the window, float32 frame arithmetic
    assert len(segs) == 1 and segs[0]["start"] == 30.0 and offset == 1234
    assert segs[0]["end"] == 30.0 + int(torch.tensor(1234) * 0.01 / 0.02) * 0.02
    segs, offset = G.retrieve_segment(_t(TB + 3, 5, 6, TB + 70), 30.0, TB, 3000, 3)   # a lone final timestamp: its time ends it
    assert len(segs) == 1 and segs[0]["end"] == 30.0 + 70.0 * 0.02 and offset == 3000
    segs, _ = G.retrieve_segment(_t(TB, 5), 0.0, TB, 3000, 3)                 # only <|0.00|>: the window length
    assert segs[0]["end"] == 1500 * 0.02
    segs, offset = G.retrieve_segment(_t(5, TB + 7, TB + 9), 0.0, TB, 3000, 3)   # a trailing pair: one segment including both
    assert [s["tokens"].tolist() for s in segs] == [[5, TB + 7, TB + 9]] and offset == 7 * 2 and segs[0]["end"] == 7 * 0.02


def test_strip_generated_follows_generate_with_fallback():
    assert G.strip_generated(_t(5, 6, 400, 400, 400), 400, 400).tolist() == [5, 6]
    assert G.strip_generated(_t(5, 6, 400), 400, 400).tolist() == [5, 6]
    assert G.strip_generated(_t(5, 6), 400, 400).tolist() == [5, 6]


def test_fixture_segments_pad_to_the_recorded_sequences():
    F = golden("generate_timestamps.npz")
    for key in [k[len("seq_"):] for k in F.files if k.startswith("seq_")]:
        seg, tok, times = F["seg_" + key], F["segtok_" + key], F["segtime_" + key]
        clips = F["seq_" + key].shape[0]
        segments = [[] for _ in range(clips)]
        for (c, a, b, i0, i1), (s, e) in zip(seg, times):
            segments[c].append({"tokens": torch.from_numpy(tok[a:b]), "start": s, "end": e, "idxs": (i0, i1)})
            assert e >= s
        out = G.pad_segments(segments, 400)
        np.testing.assert_array_equal(out.numpy(), F["seq_" + key], err_msg=key)
        for segs in segments:                                                # within a window, segments are consecutive
            for a, b in zip(segs, segs[1:]):
                assert b["start"] >= a["start"]


def test_max_frames_and_seek_and_refusals():
    mf, seek = G.max_frames_and_seek(2, torch.tensor([[1] * 5 + [0] * 3, [1] * 8]), 8, False)
    assert mf.tolist() == [5, 8] and seek.tolist() == [0, 0]
    mf, _ = G.max_frames_and_seek(2, None, 2000, True)
    assert mf.tolist() == [2000, 2000]
    with pytest.raises(ValueError, match="attention_mask"):
        G.max_frames_and_seek(2, None, 6000, False)


def test_init_tokens_drop_no_timestamps_with_timestamps():
    gc = G.GenerationConfig(decoder_start_token_id=401, lang_to_id={"<|en|>": 402}, task_to_id={"translate": 405, "transcribe": 406},
                            no_timestamps_token_id=410, language="en")
    assert G.retrieve_init_tokens(gc, 2) == [[401, 402, 406, 410]] * 2
    assert G.retrieve_init_tokens(gc, 2, return_timestamps=True) == [[401, 402, 406]] * 2


def test_timestamp_options_stay_in_extra():
    gc = G.GenerationConfig.from_dict({"return_timestamps": True, "max_initial_timestamp_index": 50, "no_timestamps_token_id": 410})
    assert "return_timestamps" not in G.FIELDS and gc.extra == {"return_timestamps": True, "max_initial_timestamp_index": 50}
    r = G.TimestampRules(400, 410, 3, gc.extra["max_initial_timestamp_index"])
    assert r.timestamp_begin == 411 and r.mii == 50 and G.TimestampRules(400, 410, 3).mii == -1


def test_frame_mask_matches_the_recorded_hf_masks():
    from mlx8_ws_audio_transformer_amd.feature_extraction import frame_attention_mask
    F = golden("generate_timestamps.npz")
    lens = [int(n) for n in F["mask_lengths"]]
    m = frame_attention_mask(lens, max(lens))
    np.testing.assert_array_equal(m, F["mask_ragged"])
    assert m.shape == (3, 3300) and m.sum(-1).tolist() == [101, 701, 3300]
    secs = [float(x) for x in F["lf_seconds"]]
    lf = [int(round(x * 16000)) for x in secs]
    assert max(lf) % 160 != 0                                                 # the fixture's last window ends on a partial frame
    np.testing.assert_array_equal(frame_attention_mask(lf, max(lf)), F["mask_lf"])
    assert frame_attention_mask([480000, 1000], 480000).shape == (2, 3000)


def test_seek_loop_on_ragged_frames_with_a_stub_decoder():
    """A batch whose longest clip is not a multiple of 160 samples: windows are sliced, then zero-padded, and every clip is seeked to
    its mask's frame count."""
    from mlx8_ws_audio_transformer_amd.feature_extraction import frame_attention_mask
    lens = [16001 * 3, 528151, 300 * 160 + 7]
    N = max(lens)
    mask = torch.from_numpy(frame_attention_mask(lens, N))
    feats = torch.randn((3, 4, N // 160))
    gc = G.GenerationConfig(eos_token_id=400, pad_token_id=400, no_timestamps_token_id=410)
    init = torch.tensor([[401, 402, 406]] * 3)
    windows = []

    def decode(seg, init_rows, max_len):
        assert seg.shape[-1] == 3000
        windows.append(seg.clone())
        gen = torch.tensor([[TB, 5, 6, 400]] * seg.shape[0])                  # <|0.00|> text...: no pair, the whole window is consumed
        return torch.cat([init_rows, gen], dim=1)
    seqs, segs = G.longform_generate(feats, mask, init, gc, 24, 64, 3000, decode, G.TimestampRules(400, 410, 3))
    assert [len(s) for s in segs] == [1, 2, 1]
    assert segs[1][1]["seek"] == 3000 and segs[1][1]["start"] == 30.0
    last = windows[1][0]                                                      # second window of the longest clip: 300 frames, then zeros
    torch.testing.assert_close(last[:, : N // 160 - 3000], feats[1, :, 3000:])
    assert bool((last[:, N // 160 - 3000:] == 0).all())
    assert seqs.shape == (3, 6)
