"""bench.py --dump-outputs: the sample of result ciphertexts it writes is fixed by the batch alone, holds the residues
exactly in float64 and stays within 64 MB at the default batch (checked on a CPU tensor; no device needed)."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_an_exact_seeded_sample(tmp_path):
    bench = _bench()
    total, n = 300, 64
    res = torch.randint(0, (1 << 50) - 1, (total, 2, bench.L, n), dtype=torch.int64, generator=torch.Generator().manual_seed(5))
    pairs = bench.dump_outputs(str(tmp_path / "a"), res)
    assert pairs == bench.dump_outputs(str(tmp_path / "b"), res)  # the same pairs every run
    assert pairs[0] == 0 and pairs[-1] == total - 1 and len(pairs) == 32 and pairs == sorted(set(pairs))
    got = np.load(tmp_path / "a" / "mul_relin_out.npy")
    assert got.dtype == np.float64 and got.shape == (32, 2, bench.L, n)
    assert np.array_equal(got.astype(np.int64), res[pairs].numpy())
    assert os.listdir(tmp_path / "a") == ["mul_relin_out.npy"]
    # small batches dump every pair
    assert bench.dump_outputs(str(tmp_path / "c"), res[:3]) == [0, 1, 2]
    # the default run (8192 pairs of [2][L][N] residues): at most 32 pairs as float64
    assert 32 * 2 * bench.L * bench.N * 8 <= 64 * 2 ** 20
