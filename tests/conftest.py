import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden():
    from safetensors.torch import load_file

    def load(name):
        path = os.path.join(GOLDEN, name)
        if os.path.exists(path):
            return load_file(path)
        # a fixture above the 1 MiB limit for a committed file is stored as <stem>.part0.safetensors, .part1, ...; a tensor
        # found in several parts was cut along its last dimension, and its pieces are joined in part order
        import torch
        stem, pieces, i = path[: -len(".safetensors")], {}, 0
        while os.path.exists(f"{stem}.part{i}.safetensors"):
            for k, t in load_file(f"{stem}.part{i}.safetensors").items():
                pieces.setdefault(k, []).append(t)
            i += 1
        if not pieces:
            raise FileNotFoundError(path)
        return {k: ts[0] if len(ts) == 1 else torch.cat(ts, dim=-1) for k, ts in pieces.items()}
    return load


def seeded(shape, seed, dtype=None, scale=1.0):
    import torch
    g = torch.Generator("cpu").manual_seed(seed)
    x = torch.randn(shape, generator=g, dtype=torch.float32) * scale
    return x.to(torch.bfloat16 if dtype is None else dtype)
