#!/usr/bin/env python3
"""tests/_losses.py's float64 restatement against the LIVE reference on random shapes (build container only; run in a
subprocess by tests/test_losses_cpu.py because the import recipe patches torch): both mask shapes, odd and tiny N, SSR labels
with void rays, gradients included."""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden as mg  # noqa: E402
import make_golden_losses as gen  # noqa: E402
import _losses  # noqa: E402


def main():
    _, helpers, _, _, _ = mg.import_reference()
    from SSR.training import training_utils as ssr_utils
    rng = np.random.default_rng(7)
    checked = 0
    for trial in range(24):
        n = int(rng.choice([2, 3, 4, 5, 7, 64, 129, 1000, 1023]))
        ssr = trial % 3 == 2
        kw = dict(classes=int(rng.integers(1, 12)), void=float(rng.uniform(0, 0.5))) if ssr else dict(mask=("vector", "outer")[trial % 2])
        case = gen.make_inputs(rng, n=n, levels=1, target=bool(trial % 4 < 2), **kw)
        case["weights"], case["levels"] = gen.WEIGHTS, 1
        fn, mse = (ssr_utils.compute_intrinsic_loss, ssr_utils.img2mse) if ssr else (helpers.compute_intrinsic_loss, helpers.img2mse)
        t_ref, total_ref, g_ref = gen.evaluate(case, 1, fn, mse, torch.float64)
        t_own, total_own, g_own = _losses.restate(case)
        assert torch.equal(torch.isnan(t_ref[0]), torch.isnan(t_own[0])), (trial, n, t_ref, t_own)
        ok = ~torch.isnan(t_ref[0])
        assert torch.allclose(t_own[0][ok], t_ref[0][ok], rtol=1e-12, atol=1e-15), (trial, n, t_ref, t_own)
        for k, g in g_ref.items():
            assert torch.allclose(g_own[k], g, rtol=1e-10, atol=1e-14), (trial, n, k)
        checked += 1
    print(f"restatement == reference on {checked} random cases")


if __name__ == "__main__":
    main()
