"""spx_edit_warp_rows and spx_edit_unwarp_rows on device memory that is not zero: the same calls once on clean outputs and once on
outputs, counts and an index region that hold a dirt pattern (tests/dirty_memory.py, unchanged), byte for byte the same rows.

Zero rows are the case that dirt shows: a row of zeros that was skipped instead of stored keeps what the buffer held."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dirty_memory as D  # noqa: E402
import edit_rows_ref as W  # noqa: E402
import tsm_inputs as I  # noqa: E402

pytestmark = pytest.mark.gpu


def _calls(b, labels, feats, hop):
    """Every row call of the batch as {name: array}; the index is built again, in whatever memory the allocator hands out."""
    b.d_index, b._index_built = None, False
    r = {}
    warped = b.warp_rows(labels, hop)
    for i in range(b.n):
        r["labels[%d]" % i] = warped[i]
        r["features[%d]" % i] = b.warp_rows(feats, hop, blend=True)[i]
        r["features_nearest[%d]" % i] = b.warp_rows(feats, hop, phase=0)[i]
    back = b.unwarp_rows(warped, hop)
    wide = b.unwarp_rows([np.repeat(w.astype(np.float64), 5, axis=1) for w in warped], hop, phase=hop - 1)
    for i in range(b.n):
        r["back[%d]" % i], r["back_wide[%d]" % i] = back[i], wide[i]
    return r


@pytest.mark.parametrize("pattern", ["7f", "ff", "random"])
def test_row_calls_on_dirty_outputs_equal_the_clean_ones(pattern):
    from speedy_amd.batch import Batch, Plan
    by = {j[0]: j for j in I.linear_jobs()}
    jobs = [by["speeds/16000Hz/1ch/9001/3.5"], by["rates/16000Hz/2ch/4800/0.4"]]
    plan = Plan(16000, False)
    try:
        b = Batch(plan, [j[3].size // j[2] for j in jobs], [j[2] for j in jobs], [j[4] for j in jobs], 0.0, edits=True)
        b.upload([j[3] for j in jobs])
        b.run()
        hop = 160
        rng = np.random.default_rng(3)
        # tracks two rows short of the input: the last sources read as rows of zeros
        rows = [max(1, -(-int(n) // hop) - 2) for n in b.lengths]
        labels = [rng.integers(1, 1 << 30, (n, 1)).astype(np.int32) for n in rows]
        feats = [rng.standard_normal((n, 7)).astype(np.float32) for n in rows]
        clean = _calls(b, labels, feats, hop)
        with D.dirty_allocations(pattern):
            dirty = _calls(b, labels, feats, hop)
        assert D.differences(clean, dirty) == []
        zero_rows = sum(int((v == 0).all(axis=1).sum()) for k, v in clean.items() if k.startswith(("labels", "back[")))
        assert zero_rows > 0, "no row of zeros among the results: the dirt would not show a skipped store"
        assert clean["labels[0]"].shape[0] == W.rows(int(b.d_nout.cpu()[0]), hop, hop // 2)
    finally:
        plan.close()
