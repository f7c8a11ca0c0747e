"""TEST INFRASTRUCTURE: weight fake-quantisation that mirrors the fp8w packing of the HIP library
(vima_amd/csrc/vima_api.hip: Packer::pack_w / fp8_eligible / f32_to_e4m3) so that the ORACLE can be run on exactly the
weights the fp8w kernels multiply with: every eligible Linear weight is replaced by dequant(quant(w)) with one scale
(amax / 448) per OUTPUT channel of the packed [N, K] matrix and OCP E4M3 round-to-nearest-even. With these weights the
oracle differs from the HIP fp8w path only by bf16 activation rounding (like the bf16 mode), which separates "is the fp8
kernel correct" (tight gate) from "how much accuracy do 3-bit-mantissa weights cost" (reported against the unmodified
reference's goldens)."""
from __future__ import annotations

import re

import torch


def eligible(N: int, K: int) -> bool:
    return K % 64 == 0 and N % 4 == 0 and N * K >= 65536


def _q_rows(w: torch.Tensor) -> torch.Tensor:
    """w [N, K] fp32 -> dequantised fp8 copy, per-row scale."""
    amax = w.abs().amax(dim=1, keepdim=True)
    scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    q = (w / scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float()
    return q * scale


LINEAR = [  # nn.Linear layout [out, in]: quantised per row
    r"obj_encoder\.cropped_img_encoder\.vit\.blocks\.\d+\.attn\.in_proj_weight$",
    r"obj_encoder\.cropped_img_encoder\.vit\.blocks\.\d+\.attn\.out_proj\.weight$",
    r"obj_encoder\.cropped_img_encoder\.vit\.blocks\.\d+\.mlp\.c_(fc|proj)\.weight$",
    r"obj_encoder\.bbox_mlp\.\w+\.[36]\.weight$",
    r"obj_encoder\.pre_transformer_layer\.\w+\.weight$",
    r"prompt_obj_post_layer\.[036]\.weight$",
    r"t5_prompt_encoder\.t5\.encoder\.block\.\d+\.layer\.0\.SelfAttention\.o\.weight$",
    r"t5_prompt_encoder\.t5\.encoder\.block\.\d+\.layer\.1\.DenseReluDense\.wo\.weight$",
    r"t5_prompt_encoder_post_layer\.weight$",
    r"xattn_gpt\.xattns\.\d+\.(query|key_value|attention_out|linear1|linear2|gated_layer)\.weight$",
    r"xattn_gpt\.h\.\d+\.mlp\.gated_layer\.weight$",
    r"action_encoder\._post_layer\.weight$",
    r"action_decoder\._decoders\.\w+\.mlps\.\d+\.0\.weight$",
]
CONV1D = [  # HF Conv1D [in, out] and `x @ projection`: quantised per column
    r"xattn_gpt\.h\.\d+\.attn\.c_(attn|proj)\.weight$",
    r"xattn_gpt\.h\.\d+\.mlp\.c_(fc|proj)\.weight$",
    r"obj_encoder\.cropped_img_encoder\.vit\.projection$",
]


def fake_quant_state_dict(sd: dict, t5_fused_rms: bool = True) -> dict:
    out = dict(sd)
    for k, w in sd.items():
        if any(re.search(p, k) for p in LINEAR):
            if eligible(w.shape[0], w.shape[1]):
                out[k] = _q_rows(w)
        elif any(re.search(p, k) for p in CONV1D):
            if eligible(w.shape[1], w.shape[0]):
                out[k] = _q_rows(w.t().contiguous()).t().contiguous()
        elif k.endswith("vit.conv1.weight"):
            out[k] = _q_rows(w.reshape(w.shape[0], -1)).reshape(w.shape)
        elif k == "obs_fusion_layer.weight":                       # packed as W[:, :E]; the 2 end-effector columns stay fp32
            E = w.shape[0]
            if eligible(E, E):
                o = w.clone()
                o[:, :E] = _q_rows(w[:, :E].contiguous())
                out[k] = o
    # T5 q / k / v (fused to one [2304, 768] GEMM: per-row scales, so fusing changes nothing) and wi: with the fused
    # RMSNorm the library quantises W diag(g); the oracle multiplies by g itself, so it gets dequant(Q(W g)) / g
    for k, w in sd.items():
        m = re.search(r"(t5_prompt_encoder\.t5\.encoder\.block\.\d+\.layer\.)(0\.SelfAttention\.[qkv]|1\.DenseReluDense\.wi)\.weight$", k)
        if not m:
            continue
        if t5_fused_rms:
            g = sd[m.group(1) + ("0" if "SelfAttention" in k else "1") + ".layer_norm.weight"]
            out[k] = _q_rows(w * g[None, :]) / g[None, :]
        else:
            out[k] = _q_rows(w)
    return out


# ---- precision "fp8": fp8 e4m3 ACTIVATIONS into the T5 stack's four GEMMs per layer, one static dequantisation scale per
# (layer, site) -- sites: 0 stream before qkv, 1 attention context, 2 stream before wi, 3 ReLU hidden (vima_api.hip t5_layer_fused with scales).
def fq_act(t: torch.Tensor, scale: float) -> torch.Tensor:
    """dequant(e4m3(t / scale)), saturating at 448, round to nearest even: what the fp8 GEMM multiplies with."""
    return (t / scale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).float() * scale


def make_fp8_act_oracle(sd: dict, act_scales: torch.Tensor, vit_scales: torch.Tensor | None = None, kv_scale: float | None = None, **ctor):
    """OraclePolicy on fake-quantised weights whose T5 stack also fake-quantises the four GEMM inputs of every layer with the
    given scales [n_layers, 4]. The RMSNorm statistics come from the UNquantised stream (the library takes them from the bf16
    stream's partial sums, vima_api.hip t5_layer_fused with scales), only the GEMM operand is quantised. `vit_scales` [4, 4]: the same for the
    ViT while the attribute `fq_vit` is True (the library quantises only chunks of >= 13824 crops: the prompt's, not one
    observation's); `kv_scale`: the prompt entering the decoder's key_value projections."""
    from .vima_oracle import OraclePolicy, FMIN, _lin, t5_relative_position_bucket

    class _Fp8ActOracle(OraclePolicy):
        fq_vit = False

        def _fq(self, group, idx, site, t):
            if group == "vit" and vit_scales is not None and self.fq_vit:
                return fq_act(t, float(vit_scales[idx, site]))
            if group == "kv" and kv_scale is not None:
                return fq_act(t, float(kv_scale))
            return t

        def _t5(self, x, mask_f):
            sdd, p = self.sd, "t5_prompt_encoder.t5.encoder."
            B, L, D = x.shape
            H, dk = 12, 64
            ext = (1.0 - mask_f[:, None, None, :]) * FMIN
            pos = torch.arange(L, device=x.device)
            bucket = t5_relative_position_bucket(pos[None, :] - pos[:, None])
            rb = sdd[p + "block.0.layer.0.SelfAttention.relative_attention_bias.weight"][bucket]
            position_bias = rb.permute(2, 0, 1).unsqueeze(0) + ext
            for l in range(act_scales.shape[0]):
                s = [float(v) for v in act_scales[l]]
                a = f"{p}block.{l}.layer.0."
                h = sdd[a + "layer_norm.weight"] * (fq_act(x, s[0]) * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-6))
                q = _lin(h, sdd[a + "SelfAttention.q.weight"]).view(B, L, H, dk).transpose(1, 2)
                k = _lin(h, sdd[a + "SelfAttention.k.weight"]).view(B, L, H, dk).transpose(1, 2)
                v = _lin(h, sdd[a + "SelfAttention.v.weight"]).view(B, L, H, dk).transpose(1, 2)
                w = torch.softmax((q @ k.transpose(3, 2) + position_bias).float(), dim=-1)
                o = (w @ v).transpose(1, 2).reshape(B, L, H * dk)
                x = x + _lin(fq_act(o, s[1]), sdd[a + "SelfAttention.o.weight"])
                f = f"{p}block.{l}.layer.1."
                h = sdd[f + "layer_norm.weight"] * (fq_act(x, s[2]) * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-6))
                h = torch.relu(_lin(h, sdd[f + "DenseReluDense.wi.weight"]))
                x = x + _lin(fq_act(h, s[3]), sdd[f + "DenseReluDense.wo.weight"])
            return self._rms(x, sdd[p + "final_layer_norm.weight"])

    return _Fp8ActOracle(fake_quant_state_dict(sd, t5_fused_rms=True), **ctor)
