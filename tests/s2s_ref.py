"""The aligner's attention decoder (ASRS2S) restated in plain torch ops, for checking the HIP training path against
torch autograd in any dtype on any device.  Not the reference's code: one function over the 14 parameters.

Per step t (Tt + 1 steps, the first on the SOS embedding, index 1; unknown-masked tokens read index 3):
  gates = W_ih [emb_t; context] + b_ih + W_hh h + b_hh;  (i, f, g, o) -> cell, h
  energies[l] = v . tanh(W_query h + W_dense conv63([w_prev; w_cum])[:, l] + W_memory memory[l]);  padded frames -inf
  w = softmax(energies);  w_cum += w;  context = w @ memory
  hidden_t = tanh(W_ph [h; context] + b_ph);  logit_t = W_pns (hidden_t * drop_scale_t) + b_pns
"""
import torch
import torch.nn.functional as F

KEYS = ("embedding.weight", "project_to_n_symbols.weight", "project_to_n_symbols.bias",
        "attention_layer.query_layer.linear_layer.weight", "attention_layer.memory_layer.linear_layer.weight",
        "attention_layer.v.linear_layer.weight", "attention_layer.location_layer.location_conv.conv.weight",
        "attention_layer.location_layer.location_dense.linear_layer.weight", "decoder_rnn.weight_ih",
        "decoder_rnn.weight_hh", "decoder_rnn.bias_ih", "decoder_rnn.bias_hh",
        "project_to_hidden.0.linear_layer.weight", "project_to_hidden.0.linear_layer.bias")


def s2s_forward(params, memory, memory_mask, tokens, unk_mask=None, drop_scale=None):
    """params: the 14 tensors in KEYS order; memory [B, L, D]; memory_mask bool [B, L] (True = padded) or None;
    tokens int [B, Tt]; unk_mask bool [B, Tt] or None; drop_scale [B, Tt + 1, D] (keep mask / (1 - p)) or None.
    Returns (hidden [B, Tt + 1, D], logit [B, Tt + 1, n_token], alignments [B, Tt + 1, L])."""
    emb, pns_w, pns_b, wq, wm, v, wloc, wdense, wih, whh, bih, bhh, ph_w, ph_b = params
    B, L, D = memory.shape
    tok = tokens.clone()
    if unk_mask is not None:
        tok[unk_mask] = 3
    tok = torch.cat([torch.ones(B, 1, dtype=tok.dtype, device=tok.device), tok], 1)
    x_all = emb[tok]  # [B, Tt + 1, E]
    pm = memory @ wm.t()
    h = memory.new_zeros(B, D)
    c = memory.new_zeros(B, D)
    ctx = memory.new_zeros(B, D)
    w = memory.new_zeros(B, L)
    cum = memory.new_zeros(B, L)
    pad = (wloc.shape[2] - 1) // 2
    hid, logit, att = [], [], []
    for t in range(tok.shape[1]):
        gates = torch.cat([x_all[:, t], ctx], 1) @ wih.t() + bih + h @ whh.t() + bhh
        i, f, g, o = gates.chunk(4, 1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        loc = F.conv1d(torch.stack([w, cum], 1), wloc, padding=pad).transpose(1, 2) @ wdense.t()  # [B, L, D]
        e = torch.tanh((h @ wq.t()).unsqueeze(1) + loc + pm) @ v.reshape(-1)
        if memory_mask is not None:
            e = e.masked_fill(memory_mask, float("-inf"))
        w = torch.softmax(e, 1)
        cum = cum + w
        ctx = (w.unsqueeze(1) @ memory).squeeze(1)
        hd = torch.tanh(torch.cat([h, ctx], 1) @ ph_w.t() + ph_b)
        hid.append(hd)
        logit.append((hd if drop_scale is None else hd * drop_scale[:, t]) @ pns_w.t() + pns_b)
        att.append(w)
    return torch.stack(hid, 1), torch.stack(logit, 1), torch.stack(att, 1)
