"""CPU-side: the size every integer-only workspace query of libawt returns, pinned byte for byte.

A workspace's size and its layout are one function in the library (csrc/common.h, Carver), so a change of a layout shows here first.  The
expected values were recorded by calling the same queries of the library built from the commit BEFORE the layouts moved onto the shared
carver (ctypes on that build's libawt.so, the shapes below, the results pasted in), i.e. they are the sizes callers have always been given.

Shapes per query: the workload's own (Whisper-small at batch 64, or the classifier's), shapes where a piece is not a multiple of 256 bytes -- every piece
that can be unaligned is unaligned in at least one row, so a layout that drops one piece's padding changes a number here -- an N that is
no multiple of 256, and the degenerate arguments that return 0.  A query takes any integers: some rows use shapes its entry point would refuse
(awt_op_linear at N = 10, K = 7; awt_op_weight_grad at N = K = 4) because only there is that piece unaligned.  The single-buffer queries are
in the table as a guard."""
import os

import pytest

from mlx8_ws_audio_transformer_amd import _lib

EXPECTED = {
    # x planes M K 2 (x2), w planes N K 2 (x2), a 256-byte flag word, the 16-row w copies ceil(N / 256) 256 K 2 (x2)
    "awt_op_linear_workspace_bytes": [
        ((96000, 2304, 768), 309068032),
        ((3, 128, 64), 99584),            # x plane 384 bytes
        ((5, 384, 64), 231168),           # N % 256 != 0: the copies cover 512 rows; x plane 640 bytes
        ((3, 10, 7), 8448),               # x plane 42, w plane 140 bytes
        ((1, 128, 64), 99072),
        ((0, 128, 64), 98560),
    ],
    # (x_rows, ldx, N, ldw): awt_op_linear's pieces with x [x_rows, ldx] and w [N, ldw] of their own pitches -- x planes x_rows ldx 2 (x2), w planes N ldw 2 (x2),
    # the flag word, the 16-row w copies ceil(N / 256) 256 ldw 2 (x2); with ldx == ldw == K it is awt_op_linear's size (the first four rows repeat its table),
    # the others are worked out by hand from that list (recorded from the commit that added the entry point: nothing precedes it)
    "awt_op_linear_fused_workspace_bytes": [
        ((96000, 768, 2304, 768), 309068032),
        ((3, 64, 128, 64), 99584),
        ((5, 64, 384, 64), 231168),
        ((3, 7, 10, 7), 8448),
        ((400, 128, 384, 384), 1581312),  # the conv stem's form: 204800 + 589824 + 256 + 786432
        ((200, 192, 256, 256), 678144),   # the LoRA form: 153600 + 262144 + 256 + 262144
        ((0, 64, 128, 64), 98560),
    ],
    # six planes of B H S 64 2 bytes
    "awt_op_attention_workspace_bytes": [
        ((64, 12, 1500), 884736000),
        ((1, 1, 3), 3072),                # plane 384 bytes
        ((1, 3, 5), 12288),               # plane 1920 bytes
        ((2, 6, 51), 470016),
        ((0, 6, 51), 0),
    ],
    # awt_op_attention's six planes, whichever outputs are asked for (its own table repeated; the single-key shape added by hand: six planes of 128 bytes)
    "awt_op_attention_ex_workspace_bytes": [
        ((64, 12, 1500), 884736000),
        ((1, 1, 3), 3072),
        ((1, 3, 5), 12288),
        ((2, 6, 51), 470016),
        ((1, 1, 1), 1536),                # plane 128 bytes
        ((0, 6, 51), 0),
        ((2, 0, 51), 0),
        ((2, 6, 0), 0),
    ],
    # eight planes of B H S 64 2 bytes: q, k, v and dO (recorded from the commit that added the entry point: nothing precedes it)
    "awt_op_attention_backward_workspace_bytes": [
        ((64, 12, 1500), 1179648000),
        ((1, 1, 3), 4096),                # plane 384 bytes
        ((1, 3, 5), 16384),               # plane 1920 bytes
        ((2, 6, 51), 626688),
        ((1, 1, 1), 2048),                # plane 128 bytes
        ((0, 6, 51), 0),
        ((2, 0, 51), 0),
        ((2, 6, 0), 0),
    ],
    # two planes of batch pad(N, 128) pad(K, 64) 2 bytes (always a multiple of 256)
    "awt_bmm_packed_bytes": [
        ((64, 1500, 768), 301989888),
        ((1, 4, 8), 32768),
        ((2, 130, 70), 262144),
        ((3, 128, 64), 98304),
        ((0, 4, 8), 0),
        ((1, 0, 8), 0),
        ((1, 4, 0), 0),
    ],
    # two planes of batch M pad(K, 64) 2 bytes
    "awt_bmm_workspace_bytes": [
        ((64, 144, 768), 28311552),
        ((1, 3, 8), 1024),                # plane 384 bytes
        ((3, 5, 70), 7680),               # plane 3840 bytes
        ((2, 4, 64), 2048),
        ((0, 3, 8), 0),
        ((1, 0, 8), 0),
        ((1, 3, 0), 0),
    ],
    # (M, rows_x, ldy, ldx, N, K): dy planes M ldy 2 (x2), x planes rows_x ldx 2 (x2), slab partials slabs N K 4
    "awt_op_weight_grad_workspace_bytes": [
        ((96000, 96000, 768, 768, 768, 768), 625213440),
        ((4, 4, 16, 8, 16, 8), 1536),     # dy plane 128, x plane 64 bytes
        ((3, 3, 8, 8, 8, 8), 1280),       # both planes 48 bytes
        ((4, 4, 16, 8, 4, 4), 1280),      # partials 64 bytes
        ((6, 9, 24, 40, 24, 40), 6400),   # dy plane 288, x plane 720, partials 3840 bytes
        ((0, 4, 16, 8, 16, 8), 0),
        ((4, 4, 16, 8, 0, 8), 0),
        ((4, 4, 16, 8, 16, 0), 0),
    ],
    # (B, T, Cin, Cout): x planes B T Cin 2 (x2), packed w planes Cout 3 Cin 2 (x2)
    "awt_op_conv1d_workspace_bytes": [
        ((16, 1024, 64, 128), 4292608),
        ((1, 3, 64, 128), 99328),         # x plane 384 bytes
        ((1, 3, 8, 4), 1024),             # x plane 48, w plane 192 bytes
        ((2, 5, 64, 384), 297472),        # Cout % 256 != 0; x plane 1280 bytes
        ((0, 3, 64, 128), 0),
        ((1, 3, 64, 0), 0),
    ],
    # one buffer: ceil(M / 256) slabs of 2 d floats (not padded)
    "awt_op_param_grad_workspace_bytes": [
        ((96000, 768), 2304000),
        ((300, 68), 1088),
        ((256, 68), 544),
        ((257, 4), 64),
        ((1, 4), 32),
        ((0, 68), 0),
    ],
    # ---- the single-buffer queries no layout function touches
    "awt_op_column_sums_ld_workspace_bytes": [((96000, 768), 1152000), ((300, 68), 544), ((1, 4), 16), ((0, 68), 0)],
    "awt_op_batchnorm_stats_workspace_bytes": [((16384, 128), 262144), ((300, 68), 2720), ((1, 4), 32), ((0, 68), 0)],
    "awt_op_bn_relu_pool_backward_workspace_bytes": [((16, 1024, 128), 262144), ((2, 150, 68), 2720), ((1, 1, 4), 32), ((0, 150, 68), 0)],
    "awt_select_tokens_workspace_bytes": [((5, 51865, 5), 9616), ((1, 51865, 1), 672), ((3, 1000, 2), 328), ((0, 51865, 5), 0)],
    "awt_select_tokens_ts_workspace_bytes": [((5, 51865, 5), 13856), ((1, 51865, 1), 1072), ((3, 1000, 2), 3520), ((0, 51865, 5), 0)],
    "awt_dtw_workspace_bytes": [((8, 448, 1500), 6981888), ((1, 3, 7), 286), ((2, 12, 100), 2944), ((0, 12, 100), 0)],
    "awt_logmel_workspace_bytes": [((64,), 256), ((1,), 256), ((65,), 512), ((0,), 256)],
}


@pytest.fixture(scope="module")
def built():
    if not os.path.exists(_lib.LIB_PATH):
        from mlx8_ws_audio_transformer_amd.build import build
        build(verbose=False)
    return _lib.lib()


@pytest.mark.parametrize("query", sorted(EXPECTED))
def test_workspace_query_returns_the_recorded_size(built, query):
    fn = getattr(built, query)
    got = [(shape, int(fn(*shape))) for shape, _ in EXPECTED[query]]
    assert got == EXPECTED[query]

