"""Shape limits of the head-grouped row kernels (csrc/headrow.h,
head_shape_ok): the attention hops of gat.py and tconv.py and the models built
on them check their shapes here."""
from __future__ import annotations

MAX_HEADS, MAX_WIDTH, MAX_FANOUT = 8, 256, 64


def check_shape(who: str, k: int, heads: int, ch: int):
    """``who`` (a hop or a model) names the caller in the error text."""
    if not (1 <= heads <= MAX_HEADS and ch >= 4 and ch % 4 == 0 and heads * ch <= MAX_WIDTH
            and 1 <= k <= MAX_FANOUT):
        raise ValueError(f"{who}: heads <= {MAX_HEADS}, channels per head a multiple of 4, heads "
                         f"* channels <= {MAX_WIDTH} and 1 <= fanout <= {MAX_FANOUT} (got k={k}, "
                         f"heads={heads}, channels={ch})")
