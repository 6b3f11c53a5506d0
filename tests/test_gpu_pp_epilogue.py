"""GPU: the ping-pong GEMM's epilogue (gemm_pp_kernel, csrc/gemm.hip) where its workgroups are PERSISTENT -- more tiles than compute units, so that
some workgroups run two tiles and the next tile's K-tile stream is in flight while a tile's strips are stored.  That is the state in which the
epilogue's registers are tight: its lane-derived addresses are formed per tile (lane_here), the fp32 rows are addressed by a wave-uniform row pointer
plus one per-lane offset (RowOff8), and every wait for a residual row is counted against the loads and stores issued after it.

Shapes: K = 128 and 192 (2 and 3 K-tile pairs, the shortest K loops the kernel takes: the next tile's first K-tiles are requested during the epilogue),
N = 256 and 768, M = 256 x (ceil(CUs / (N / 256)) + 1) read from the device (a few tiles more than compute units), and the same with 37 rows fewer
(the ragged path of the last row panel).  Epilogues: EPI_F32_RESID, EPI_BF16_GELU into split lines, EPI_F32, all through awt_op_linear_fused with
gemm_pp = 2.  Each launch is compared
  * bit for bit, every row, with the 128 x 256 kernel's launch of the same problem (gemm_f8s_kernel: the same products in the same order), and
  * with float64 (tests/gemm_reference.py) under test_gpu_gemm_epilogues' bound, on every 19th row plus the whole last row panel (the reference of all
    rows would take the test's time; 19 is coprime to every strip, tile and panel size, so every row position of a tile is sampled).
The residual is a canary: row m holds m + column / 1024, so a strip that consumed another row's residual, or one that had not landed, is off by at
least 1 where the bound is below 0.1.  Guard rows, rows >= M and the sentinel check are those of test_gpu_gemm_epilogues.launch."""
import pytest
import torch

from tests import gemm_reference as ref
from tests.test_gpu_gemm_epilogues import Worst, decode, launch, route, same_bytes, untouched

pytestmark = pytest.mark.gpu

RAGGED = 37
PP, TILE256 = {"gemm_pp": 2}, {"gemm_tile": 256}


def persistent_rows(N):
    """M with a few more 256 x 256 tiles than the device has compute units."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles_n = N // 256
    return 256 * ((cus + tiles_n - 1) // tiles_n + 1), cus


def canary(M, N):
    return (torch.arange(M, dtype=torch.float64)[:, None] + torch.arange(N, dtype=torch.float64)[None, :] / 1024.0).float()


def sample_rows(M):
    last_panel = (M - 1) // 256 * 256
    return torch.unique(torch.cat([torch.arange(0, M, 19), torch.arange(last_panel, M)]))


@pytest.mark.parametrize("K", [128, 192])
@pytest.mark.parametrize("N", [256, 768])
def test_persistent_ping_pong_epilogues(N, K):
    M_full, cus = persistent_rows(N)
    assert M_full // 256 * (N // 256) > cus, "some workgroup must run a second tile"
    x, w, b = ref.make_inputs(M_full, N, K, 91)
    resid_full, worst = canary(M_full, N), Worst()
    for M in (M_full, M_full - RAGGED):
        p = ref.Problem(x[:M].contiguous(), w, b)
        rows = sample_rows(M)
        ps = ref.Problem(p.x[rows].contiguous(), w, b)
        assert route(5, M, N, K, pp=2) == "pp" and route(5, M, N, K, tile=256) == "f8s"
        for epi, ilv in (("f32_resid", False), ("gelu", True), ("f32", False)):
            side = {"resid": resid_full[:M]} if epi == "f32_resid" else {}
            r = launch(p, epi, 5, PP, side, split_lines=ilv)
            untouched(r)
            tiles128 = launch(p, epi, 5, TILE256, side)
            untouched(tiles128)
            assert same_bytes(r, tiles128), f"{epi} M={M} N={N} K={K}: ping-pong and 128 x 256 tiles differ"
            ex, tol = ref.bound(ps, epi, 5, **({"resid": resid_full[:M][rows]} if epi == "f32_resid" else {}))
            if epi == "f32_resid":
                assert tol["y"] < 0.1, tol                                      # the canary's step is 1
            got = {name: v[rows] for name, v in decode(r).items()}
            worst.add(epi, "pp_lines" if ilv else "pp", ref.check(f"persistent {epi} M={M} N={N} K={K}", got, ex, tol))
    worst.report(f"persistent N={N} K={K}")
