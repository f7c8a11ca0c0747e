"""Which options end a running episode batch (vima_set_option against the handle's one episode state), on the MI355X. The rules are the ones
the library has always had; nothing else held them:

  decode_ring    ends the running episode of every handle kind;
  kv_headmajor   ends the XAttnGPT episode (vima_decode_step) and drops the prompt K / V cache; a decoder-only episode goes on;
  seq_ring       ends the decoder-only episode (vima_seq_prefill / vima_seq_decode_step); an XAttnGPT episode goes on.

"Ends": the next step is refused with "does not continue the episode state" and nothing is launched. "Goes on": the next step returns the bytes
it returns without the option call. VIMA: syn.config("2M") in bf16, B = 2, Q = 2, Lp = 4 on random tokens; decoder-only: the GPT case of
oracle/cases.py (B = 3, Q = 1)."""
import pytest
import torch

from oracle.cases import baseline_state_dict, build_baseline_case
from tests.gpu_common import loaded_policy
from vima_amd import _lib
from vima_amd.baselines import build_baseline
from vima_testing import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, Q, LP = 2, 2, 4
REFUSED = "does not continue the episode state"


def _vima_policy():
    cfg = syn.config("2M")
    return loaded_policy(cfg, syn.make_state_dict(cfg, 7, head_gain=0.5), "bf16")


@pytest.fixture(scope="module")
def vima():
    return _vima_policy()


@pytest.fixture(scope="module")
def vima_tokens(vima):
    g, E = torch.Generator().manual_seed(11), vima.embed_dim
    return dict(obs=torch.randn(3, B, Q, E, generator=g).to(DEV), mask=torch.ones(B, Q, dtype=torch.bool, device=DEV),
                act=torch.randn(3, B, E, generator=g).to(DEV), prompt=torch.randn(LP, B, E, generator=g).to(DEV),
                pmask=torch.ones(B, LP, dtype=torch.bool, device=DEV))


def _step(pol, tok, t):
    return pol.forward_step(tok["obs"][t], tok["mask"], tok["act"][t - 1] if t else None, tok["prompt"], tok["pmask"], t)


def test_seq_ring_does_not_end_an_xattngpt_episode(vima, vima_tokens):
    twin = _vima_policy()                                            # never sets the option
    for t in (0, 1):
        assert torch.equal(_step(vima, vima_tokens, t), _step(twin, vima_tokens, t))
    vima.set_option("seq_ring", 1)
    try:
        got, want = _step(vima, vima_tokens, 2), _step(twin, vima_tokens, 2)
        torch.cuda.synchronize()
        assert torch.isfinite(want).all() and torch.equal(got, want)
    finally:
        vima.set_option("seq_ring", 0)


@pytest.mark.parametrize("option,value,restore", [("decode_ring", 1, 0), ("decode_ring", 0, 0), ("kv_headmajor", 0, 1), ("kv_headmajor", 1, 1)])
def test_option_ends_an_xattngpt_episode(vima, vima_tokens, option, value, restore):
    for t in (0, 1):
        _step(vima, vima_tokens, t)
    vima.set_option(option, value)
    try:
        with pytest.raises(_lib.VimaError, match=REFUSED):
            _step(vima, vima_tokens, 2)
    finally:
        vima.set_option(option, restore)
    assert torch.isfinite(_step(vima, vima_tokens, 0)).all()         # a new episode starts with step 0


@pytest.fixture(scope="module")
def gpt():
    cfg, prompts, obs, actions = build_baseline_case("baseline_gpt")
    pol = build_baseline(cfg, precision="bf16", device=DEV)
    pol.load_state_dict(baseline_state_dict("baseline_gpt", cfg), strict=True)
    with torch.no_grad():
        ptok, pmask = pol.forward_prompt_assembly(syn.to_device(prompts, DEV))
        otok = pol.forward_obs_token(syn.to_device(obs, DEV))       # [T, B, Q, E]
        atok = pol.forward_action_token(syn.to_device(actions, DEV))
    return pol, ptok, pmask, otok, atok


@pytest.mark.parametrize("option,value", [("decode_ring", 0), ("seq_ring", 1), ("seq_ring", 0)])
def test_option_ends_a_decoder_only_episode(gpt, option, value):
    pol, ptok, pmask, otok, atok = gpt
    pol.seq_prefill(ptok, pmask)
    pol.seq_step(otok[0])
    pol.set_option(option, value)
    try:
        with pytest.raises(_lib.VimaError, match=REFUSED):
            pol.seq_step(otok[1], atok[0])
    finally:
        pol.set_option("seq_ring", 0)


def test_kv_headmajor_does_not_end_a_decoder_only_episode(gpt):
    pol, ptok, pmask, otok, atok = gpt
    outs = []
    for flip in (False, True):
        pol.seq_prefill(ptok, pmask)
        pol.seq_step(otok[0])
        if flip:
            pol.set_option("kv_headmajor", 0)
        outs.append(pol.seq_step(otok[1], atok[0]))
    pol.set_option("kv_headmajor", 1)
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
