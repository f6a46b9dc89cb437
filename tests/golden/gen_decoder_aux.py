"""Generate tests/golden/decoder_aux.npz from the IMPORTED REFERENCE (build container only): the whole of res_aux -- vel, cov_vel, param --
under both curve bases of SceneDecoder (param_out 'bezier' / 'monomial', network.py:408-435, :514-534), for formula weights and formula
inputs, so that only expected outputs are stored.  Re-run:  python tests/golden/gen_decoder_aux.py

Keys: "<basis>_a<a>_l<l>_b<B>_s<seed>_{cls,reg,vel,cov_vel,param}"; cls [B,6], reg [A,6,60,5], vel [A,6,60,2], cov_vel [A,6,60,3], param
[A,6,8,5] (the reference's [6,a,8,5] per scene, transposed to agent-major and concatenated over the scenes).
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np
import torch

GOLD = os.path.join(ROOT, "tests", "golden")
PATH = os.path.join(GOLD, "decoder_aux.npz")
BASES = ("bezier", "monomial")
CASES = [(3, 4, 2, 1), (2, 2, 1, 3), (5, 6, 3, 2)]      # (a, l, B, seed)
REG_MAX = 50.0      # exp of a monomial sum can be large, and an absolute tolerance means nothing there: pick another seed if a case trips this


def case_key(basis, case):
    return "%s_a%d_l%d_b%d_s%d" % ((basis,) + tuple(case))


def build_ref_network(sd, param_out):
    """the reference ScenePredNet on the CPU, eval mode, as oracle/ref_harness.build_ref_network builds it, with cfg["param_out"] set"""
    from oracle import ref_harness as rh
    m = rh.ref_modules()
    cfg = m["planners.mind.configs.networks.net_cfg"].NetCfg().get_net_cfg()
    cfg["param_out"] = param_out
    net = m["planners.mind.networks.network"].ScenePredNet(cfg, torch.device("cpu"))
    missing, unexpected = net.load_state_dict(sd)
    assert not missing and not unexpected, (missing, unexpected)
    net.eval()
    return net, m["planners.mind.utils"].get_rpe


def generate():
    """-> dict of arrays (what the committed file holds)"""
    from mind_amd.synth import predictor_batch
    from mind_amd.weights import formula_state_dict
    sd = formula_state_dict(as_torch=True)
    out = {}
    for basis in BASES:
        net, get_rpe = build_ref_network(sd, basis)
        for case in CASES:
            a, l, B, seed = case
            pb = predictor_batch(a, l, B, seed=seed)
            pb = {k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else [torch.from_numpy(x) for x in v]) for k, v in pb.items()}
            rpes = [{"scene": get_rpe(c, v)[0], "scene_mask": None} for c, v in zip(pb["CTRS"], pb["VECS"])]
            data = (pb["ACTORS"], pb["ACTOR_IDCS"], pb["LANES"], pb["LANE_IDCS"], rpes, pb["TGT_NODES"], pb["TGT_RPE"])
            with torch.no_grad():
                rc, rr, ra = net(data)
            key = case_key(basis, case)
            out[key + "_cls"] = np.stack([c.numpy()[0] for c in rc]).astype(np.float32)
            out[key + "_reg"] = np.concatenate([r.numpy() for r in rr]).astype(np.float32)
            out[key + "_vel"] = np.concatenate([x[0].numpy() for x in ra]).astype(np.float32)
            out[key + "_cov_vel"] = np.concatenate([x[1].numpy() for x in ra]).astype(np.float32)
            out[key + "_param"] = np.concatenate([x[2].permute(1, 0, 2, 3).numpy() for x in ra]).astype(np.float32)
            A = out[key + "_reg"].shape[0]
            assert out[key + "_cov_vel"].shape == (A, 6, 60, 3) and out[key + "_param"].shape == (A, 6, 8, 5), key
            assert np.abs(out[key + "_reg"]).max() < REG_MAX, (key, np.abs(out[key + "_reg"]).max())
    return out


if __name__ == "__main__":
    torch.manual_seed(0)
    out = generate()
    np.savez_compressed(PATH, **out)
    for basis in BASES:
        k = case_key(basis, CASES[0])
        print(k, "max|reg| %.3f max|cov_vel| %.3f" % (np.abs(out[k + "_reg"]).max(), np.abs(out[k + "_cov_vel"]).max()))
    print("decoder_aux.npz", sum(v.nbytes for v in out.values()) // 1024, "KiB raw,", os.path.getsize(PATH) // 1024, "KiB on disk")
