"""The life of a sum window (the metric window, the evaluation's, FQE's value pass), shared by the three files that test them: attach, two
passes, a read that keeps the sums, one that empties them, a read of the empty window, detach; and the buffers the attach call refuses."""
import numpy as np
import pytest
import torch

B = 259          # a ragged second chunk of every 256-row kernel behind the windows


def engine(kind, act_dim=2):
    from exorl_amd import _lib as L
    from exorl_amd.engine import AgentEngine
    O = 5
    eng = AgentEngine(kind, O, act_dim, 8, B, precision='fp32')
    gen = torch.Generator().manual_seed(11)
    for net in (L.NET_ACTOR, L.NET_CRITIC):
        flat = eng.flat(net)
        flat.copy_(0.3 * torch.randn(flat.numel(), generator=gen))
    eng.params_changed(sync_target=True)
    eng.set_batch(*[torch.randn(n, generator=gen) for n in (B * O, B * act_dim, B, B, B * O)])
    return eng


def check_window(eng, name, one_pass, count_per_pass, no_window):
    """name: 'metric_window', 'eval' or 'fqe_value' (AgentEngine's set_<name> / <name>_read / <name>_bytes, with the metric window's set
    spelled set_metric_window); one_pass() adds to the window; count_per_pass: what one pass adds to the count; no_window: the read's refusal."""
    from exorl_amd import _lib as L
    attach, read, nbytes = getattr(eng, f'set_{name}'), getattr(eng, f'{name}_read'), getattr(eng, f'{name}_bytes')()
    assert nbytes > 256 and nbytes % 256 == 0
    prefix = f'agent_set_{name}: buffer'
    with pytest.raises(L.ExorlError, match=prefix):         # misaligned
        attach(torch.empty(nbytes + 256, dtype=torch.uint8, device='cuda')[1:])
    with pytest.raises(L.ExorlError, match=prefix):         # short
        attach(torch.empty(nbytes, dtype=torch.uint8, device='cuda')[:nbytes - 1])
    with pytest.raises(L.ExorlError, match=no_window):      # a refused buffer attaches nothing
        read()
    attach(torch.full((nbytes,), 0xFF, dtype=torch.uint8, device='cuda'))
    one_pass(), one_pass()
    sums, count = read(reset=False)
    assert count == 2 * count_per_pass and np.isfinite(sums).all() and np.abs(sums).sum() > 0
    again, count2 = read(reset=True)
    assert count2 == count and again.tobytes() == sums.tobytes()
    empty, count3 = read(reset=True)
    assert count3 == 0 and not empty.any()
    attach(None)
    with pytest.raises(L.ExorlError, match=no_window):
        read()
