"""Cross-check of the oracle against the unmodified reference (imported through oracle/ref_shim.py) on a case that is not in the
golden set. What the reference computed for it is stored in tests/golden/reference_9M_masked.npz (written by
`python -m tests.test_oracle_vs_reference --write-golden` where the reference tree is present), so the check runs anywhere;
where the reference tree is present it is also run live."""
import os
import sys

import numpy as np
import torch

from oracle import ref_shim
from oracle.cases import run_policy
from oracle.vima_oracle import OraclePolicy
from vima_testing import synthetic as syn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_9M_masked.npz")


def _case():
    """9M model (E=320, 10 heads), batch 2, different seeds, prompt with a padded tail."""
    cfg = syn.config("9M")
    sd = syn.make_state_dict(cfg, seed=11)
    prompts = syn.make_prompt(2, layout=[[0, 1, 0, 0], [0, 0, 1, 0, 1, 0, 0]], q_per_view=2, seed=99)
    obs = syn.make_obs(2, 2, 2, seed=98)
    actions = syn.make_actions(1, 2, seed=97)
    return cfg, sd, prompts, obs, actions


def _reference_live(cfg, sd, prompts, obs, actions):
    """-> (outputs, action modes) of the reference policy."""
    pol = ref_shim.build_reference_policy(**cfg.ctor_kwargs())
    pol.load_state_dict(sd, strict=True)
    ref_out, ref_d = run_policy(pol, prompts, {"objects": ref_shim.MapDict(obs["objects"]), "ee": obs["ee"]}, actions)
    return ref_out, {k: d.mode() for k, d in ref_d.items()}


def _reference_stored():
    g = np.load(GOLDEN)
    pick = lambda p: {k[len(p):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(p)}   # noqa: E731
    return pick("out."), pick("mode.")


def test_live_reference_matches_oracle_masked_prompt():
    cfg, sd, prompts, obs, actions = _case()
    orc = OraclePolicy(sd, **cfg.ctor_kwargs())
    out, d = run_policy(orc, prompts, obs, actions)
    refs = [_reference_stored()]
    if ref_shim.reference_available():
        refs.append(_reference_live(cfg, sd, prompts, obs, actions))
    for ref_out, ref_modes in refs:
        assert sorted(ref_out) == sorted(out) and sorted(ref_modes) == sorted(d)
        for k in ref_out:
            if ref_out[k].dtype == torch.bool:
                assert torch.equal(ref_out[k], out[k]), k
            else:
                assert (ref_out[k] - out[k]).abs().max().item() < 5e-5, k
        for k in ref_modes:
            assert torch.equal(ref_modes[k], d[k]["mode"]), k


def _write_golden():
    ref_out, ref_modes = _reference_live(*_case())
    arrays = {f"out.{k}": v.numpy() for k, v in ref_out.items()}
    arrays.update({f"mode.{k}": v.numpy() for k, v in ref_modes.items()})
    np.savez_compressed(GOLDEN, **arrays)
    print("wrote", GOLDEN, {k: v.shape for k, v in arrays.items()})


if __name__ == "__main__":
    if "--write-golden" in sys.argv:
        _write_golden()
