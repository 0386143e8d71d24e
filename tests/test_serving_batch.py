"""/generate_batch of the serving example over the FastAPI test client:
ragged prompts round-trip, greedy rows match /generate, malformed bodies
are rejected. Tiny GPT-2-shaped model on CPU."""

import pytest
import torch

fastapi = pytest.importorskip("fastapi")
from fastapi.testclient import TestClient

from tnn_amd.nn import LayerBuilder

PROMPTS = [[1, 2, 3], [4], [5, 6, 7, 8, 9, 10, 11]]


@pytest.fixture(scope="module")
def client():
    import examples.serve_gpt2 as srv
    from tnn_amd.models import register_model

    @register_model("tiny_gpt2_serving_batch")
    def tiny(dtype=torch.float32):
        return (LayerBuilder((16,), dtype)
                .embedding(128, 32)
                .positional_embedding(64, 32)
                .gpt_block(32, 2, flash=False)
                .gpt_block(32, 2, flash=True)
                .layernorm()
                .dense(128, True, "head")
                .build("tiny_gpt2_serving_batch"))

    torch.manual_seed(0)
    app = srv.build_app("tiny_gpt2_serving_batch", seq_len=64, device="cpu")
    return TestClient(app)


def test_generate_batch_round_trip(client):
    r = client.post("/generate_batch", json={"prompts": PROMPTS,
                                             "max_new_tokens": 5})
    assert r.status_code == 200
    body = r.json()
    assert len(body["ids"]) == len(body["new_ids"]) == len(PROMPTS)
    for p, ids, new in zip(PROMPTS, body["ids"], body["new_ids"]):
        assert ids == p + new
        assert 1 <= len(new) <= 5 and all(0 <= t < 128 for t in new)
    assert body["tokens_per_s"] > 0


def test_generate_batch_greedy_matches_generate(client):
    body = client.post("/generate_batch", json={"prompts": PROMPTS,
                                                "max_new_tokens": 6}).json()
    for p, ids in zip(PROMPTS, body["ids"]):
        one = client.post("/generate", json={"ids": p, "max_new_tokens": 6})
        assert one.json()["ids"] == ids


def test_generate_batch_sampling_is_seeded(client):
    req = {"prompts": PROMPTS, "max_new_tokens": 6, "greedy": False,
           "temperature": 1.3, "top_k": 30, "top_p": 0.95, "seed": 4}
    a = client.post("/generate_batch", json=req).json()["ids"]
    assert client.post("/generate_batch", json=req).json()["ids"] == a
    b = client.post("/generate_batch", json=dict(req, seed=5)).json()["ids"]
    assert a != b


@pytest.mark.parametrize("body", [
    {}, {"prompts": []}, {"prompts": [[1], []]}, {"prompts": [[1, -2]]},
    {"prompts": "abc"}, {"prompts": [[1, "x"]]},
    {"prompts": [[1]], "top_p": 0.0}, {"prompts": [[1]], "top_k": -3},
    {"prompts": [[1]], "greedy": False, "temperature": -1.0},
])
def test_generate_batch_rejects_malformed(client, body):
    assert client.post("/generate_batch", json=body).status_code in (400, 422)
