"""Drop-ins for utils.py:14-27 `maximum_path` and monotonic_align's `mask_from_lens`: the monotonic alignment search
of train.py:213-214 on the HIP path (stts_maximum_path), without the device -> host -> device round trip of the
Cython core.  The lengths are read on the host (as the reference reads them) and checked there: the search is
undefined for tx > ty or tx < 1.
"""
from __future__ import annotations

import ctypes

import torch

from . import engine as E


def mask_from_lens(attn, text_lens, mel_lens):
    """monotonic_align.mask_from_lens: bool [B, T_text, T_mel] (attn's last two axes), True inside each utterance's
    (text_lens[b], mel_lens[b]) rectangle."""
    Tx, Ty = attn.shape[-2], attn.shape[-1]
    dev = attn.device
    tx = torch.arange(Tx, device=dev)[None, :, None] < text_lens.to(dev)[:, None, None]
    ty = torch.arange(Ty, device=dev)[None, None, :] < mel_lens.to(dev)[:, None, None]
    return tx & ty


def maximum_path(neg_cent, mask):
    """neg_cent [B, T_text, T_mel], mask of the same shape -> the 0 / 1 path in neg_cent's dtype and on its device;
    rows tx = mask.sum(1)[:, 0], columns ty = mask.sum(2)[:, 0], as utils.py:24-25."""
    if neg_cent.dim() != 3 or tuple(mask.shape) != tuple(neg_cent.shape):
        raise ValueError(f"maximum_path: neg_cent {tuple(neg_cent.shape)}, mask {tuple(mask.shape)}")
    B, Tx, Ty = neg_cent.shape
    # (utils.py's names are swapped: its t_t_max = mask.sum(1)[:, 0] counts the rows, the text axis)
    lens = torch.stack([mask.sum(1)[:, 0], mask.sum(2)[:, 0]]).to(torch.int32).cpu()
    tx, ty = lens[0].tolist(), lens[1].tolist()
    for b in range(B):
        if tx[b] < 1 or tx[b] > ty[b]:
            raise ValueError(f"maximum_path: utterance {b} has {tx[b]} tokens for {ty[b]} frames; the search needs "
                             "1 <= tokens <= frames")
    E._require_device()
    dev = neg_cent.device if neg_cent.is_cuda else torch.device("cuda", torch.cuda.current_device())
    value = E._dev_f32(neg_cent, dev)
    path = torch.empty(B, Tx, Ty, dtype=torch.float32, device=dev)
    arr = ctypes.c_int * B
    E.call("stts_maximum_path", value, arr(*tx), arr(*ty), B, Tx, Ty, path,
           ws=("stts_maximum_path_workspace_bytes", B, Tx, Ty))
    return path.to(device=neg_cent.device, dtype=neg_cent.dtype)
