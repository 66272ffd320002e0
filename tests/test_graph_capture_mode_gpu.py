"""A hipGraph captured outside inference mode while an engine that captured its decode graphs is alive. The first live
graph of a process makes torch create the default generator's graph-state tensors when its capture begins; the engine
runs its steps in inference mode, and tensors created there are inference tensors, on which a capture begun outside
inference mode fails (an in-place fill). engine/graphs.py therefore begins its captures outside inference mode."""
import pytest
import torch

from kafka_llm_service_amd.engine.engine import EngineConfig, LLMEngine
from kafka_llm_service_amd.engine.sequence import SamplingParams


@pytest.mark.gpu
def test_capture_outside_inference_mode_beside_a_graphed_engine(cuda):
    eng = LLMEngine(EngineConfig(model="tiny-llama", device="cuda:0", num_kv_blocks=512, max_model_len=2048,
                                 use_graphs=True))
    out = eng.generate([[1, 2, 3, 4, 5]], SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True))
    assert len(out[0]) == 6 and not eng.runner.graphs.disabled and eng.runner.graphs.stats["captures"] >= 1
    x = torch.ones(8, device=cuda)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):  # (the engine and its graphs are still alive here)
        y = x * 2
    x.fill_(3.0)
    g.replay()
    torch.cuda.synchronize()
    assert y.tolist() == [6.0] * 8
    again = eng.generate([[1, 2, 3, 4, 5]], SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True))
    assert again == out and eng.runner.graphs.stats["replays"] > 0
