"""Measures, on the CPU, what tests/test_gpu_waveform_classifier.py::test_training_step_matches_autograd_of_the_restated_module rests on.
Per size (batch, N) and seed: the fp64 restatement's distance from its kinks in each conv block (smallest |z| at a BatchNorm output, smallest
margin between the two largest z of a pooling window with a positive maximum) -- the test takes the first seed with every margin above 1e-5.
For that seed: how far the fp32 torch restatement of the training step is from the fp64 one, per tensor.  The test's gradient bounds are
max(2e-4 max|grad| + 1e-7, 8 x these figures); the printed dict is pasted into the test (FP32_VS_FP64).  No GPU, no native code.

    python tools/waveform_cnn_fp32_vs_fp64.py [--full]        (--full: also the margins at N = 64000, where no parity is asserted)
"""
import copy
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import test_gpu_waveform_classifier as t  # noqa: E402


def margins(batch, N, seeds):
    for seed in seeds:
        m = t.kink_margins(t._reference(seed).double(), t._wave("wave.xt", batch, N, seed))
        print(f"# {(batch, N)} seed {seed}: " + "  ".join(f"block {i + 1}: min|z| {a:.2e} min margin {b:.2e}" for i, (a, b) in enumerate(m)), file=sys.stderr)


def measure(batch, N):
    seed = t.step_seed(batch, N)
    margins(batch, N, range(seed + 1))
    ref32 = t._reference(seed)
    ref64 = copy.deepcopy(ref32).double()
    x, y = t._wave("wave.xt", batch, N, seed), t._labels(batch)
    l64, g64 = t._train_step_reference(ref64, x, y)
    ref32.train()
    l32 = t.F.cross_entropy(ref32.classifier(ref32.conv_layers(x)), y)
    l32.backward()
    out = {"seed": seed, "loss": abs(float(l32.detach()) - float(l64))}
    for n, p in ref32.named_parameters():
        out[n] = float((p.grad.double() - g64[n]).abs().max())
        print(f"# {(batch, N)} {n}: |fp32 - fp64| {out[n]:.3e}  max|grad| {float(g64[n].abs().max()):.3e}  project bound "
              f"{2e-4 * float(g64[n].abs().max()) + 1e-7:.3e}", file=sys.stderr)
    return out


if __name__ == "__main__":
    if "--full" in sys.argv:
        margins(2, 64000, range(4))
    table = {k: measure(*k) for k in [(3, 4160), (4, 1375)]}
    print("FP32_VS_FP64 = {")
    for k, v in table.items():
        print(f"    {k}: {{" + ", ".join(f'"{n}": {e}' if n == "seed" else f'"{n}": {e:.2e}' for n, e in v.items()) + "},")
    print("}")
