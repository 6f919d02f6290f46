"""Seeded captions of a chosen token count for the GroundingDINO tests (no GPU code, nothing from the product package).

The reference builds the caption from the whole category list of the image's dataset (roi_heads_gdino.py:130-131,176-181): often
more than 100 tokens, up to max_text_len = 256. `caption_ids(T, seed)` gives such a caption as token ids: [CLS] = 101, then phrases
of 1 to 3 word ids from [200, 1000), each closed by the delimiter 1012 ('.'), then [SEP] = 102 - exactly T tokens.

ENGINE_T lists the lengths the engine tests run, each at a boundary of the native path:
   64  8 heads x 64 tokens: the last length the row-chain decoder takes with the real head count (heads * T <= 516)
  129  4 heads x 129 tokens = 516: the row chain's score region exactly full with the test model's 4 heads
  130  the first length the 4-head row chain declines (launch-per-op decoder, text cross-attention through attn_f32 with Tk = T)
  147  a second key chunk (attn_f32 walks 144 keys at a time) with T % 4 != 0: scalar bias reads, and a query whose first chunk is
       entirely masked
  256  max_text_len: second chunk with float4 bias reads, many such queries
"""
import random

import torch

CLS, SEP, DELIM = 101, 102, 1012
KEY_CHUNK = 144                     # keys per LDS chunk of attn_f32_kernel (kKC)
ENGINE_T = (64, 129, 130, 147, 256)


def caption_ids(T: int, seed: int = 0):
    """list of exactly T token ids: [101] + phrases (1..3 ids from [200, 1000), then 1012) + [102]; T >= 4."""
    if T < 4:
        raise ValueError("a caption needs [CLS], one phrase of at least one word, its delimiter and [SEP]")
    rng = random.Random(1000003 * seed + T)
    ids, left = [CLS], T - 2
    while left > 0:
        # a phrase takes n + 1 slots; never leave exactly one slot (no phrase fits it)
        choices = [n for n in (1, 2, 3) if n + 1 <= left and left - (n + 1) != 1]
        n = rng.choice(choices)
        ids += [rng.randrange(200, 1000) for _ in range(n)] + [DELIM]
        left -= n + 1
    ids.append(SEP)
    assert len(ids) == T
    return ids


def phrase_mask(ids) -> torch.Tensor:
    """bool [T][T]: token i may attend token j (same phrase, delimiter included; [CLS] / [SEP] only themselves). Written on its own,
    from the caption's structure; the CPU test holds it against HF's generate_masks_with_special_tokens_and_transfer_map."""
    T = len(ids)
    block = torch.zeros(T, dtype=torch.int64)
    b = 0
    for i, t in enumerate(ids):
        block[i] = b
        if t in (CLS, SEP, DELIM):
            b += 1
    return block[:, None] == block[None, :]


def additive_mask(mask: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """0 where attended, finfo(float32).min elsewhere: what BERT and the encoder's text self-attention add to the scores."""
    return torch.where(mask, 0.0, torch.finfo(torch.float32).min).to(dtype)


def blind_rows(mask: torch.Tensor, chunk: int = KEY_CHUNK) -> int:
    """queries whose first `chunk` keys are all masked: for them attn_f32's running maximum is still -inf after the first chunk"""
    return int((~mask[:, :chunk].any(dim=1)).sum())
