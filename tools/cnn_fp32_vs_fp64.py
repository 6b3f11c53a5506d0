"""Measures, on the CPU, how far the fp32 torch restatement of the CNN classifier's training step is from the fp64 one, per tensor, for the
inputs of tests/test_gpu_cnn_classifier.py::test_training_step_matches_autograd_of_the_restated_module.  The test's gradient bounds are
max(2e-4 max|grad| + 1e-7, 8 x these figures); the printed dict is pasted into the test (FP32_VS_FP64).  No GPU, no native code.

    python tools/cnn_fp32_vs_fp64.py
"""
import copy
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import test_gpu_cnn_classifier as t  # noqa: E402


def measure(n_mels, T, batch):
    ref32 = t._reference(n_mels, seed=7 + T)
    ref64 = copy.deepcopy(ref32).double()
    x, y = t._mel("cnn.xt", batch, n_mels, T, 5), t._labels(batch)
    l64, g64 = t._train_step_reference(ref64, x, y)
    ref32.train()
    l32 = t.F.cross_entropy(ref32.classifier(ref32.conv_layers(x)), y)
    l32.backward()
    out = {"loss": abs(float(l32.detach()) - float(l64))}
    for n, p in ref32.named_parameters():
        out[n] = float((p.grad.double() - g64[n]).abs().max())
        print(f"# {(n_mels, T, batch)} {n}: |fp32 - fp64| {out[n]:.3e}  max|grad| {float(g64[n].abs().max()):.3e}  project bound "
              f"{2e-4 * float(g64[n].abs().max()) + 1e-7:.3e}", file=sys.stderr)
    return out


if __name__ == "__main__":
    table = {k: measure(*k) for k in [(64, 126, 4), (128, 501, 2)]}
    print("FP32_VS_FP64 = {")
    for k, v in table.items():
        print(f"    {k}: {{" + ", ".join(f'"{n}": {e:.2e}' for n, e in v.items()) + "},")
    print("}")
