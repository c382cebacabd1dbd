"""The host side of the training step's status word (no GPU): the check_status contract, the bitwise-OR merge helper, the
word derived from loss terms, and the OR collective over two gloo ranks.  The device side is tests/test_status_gpu.py."""
import os
import warnings

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from openobj_amd import dist as odist
from openobj_amd import ops
from openobj_amd.render_rays import LossExplode, check_status

FORMS = {"int": lambda s: s, "0-d tensor": lambda s: torch.tensor(s, dtype=torch.int32),
         "1-element tensor": lambda s: torch.tensor([s], dtype=torch.int32)}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("word", [0, 1, 2, 3])
def test_check_status_table(word, form):
    """bit 0 raises LossExplode (the reference exits, render_rays.py:109-111) whether or not bit 1 is set with it; bit 1
    alone warns and returns the word; 0 is silent.  The same for a Python int, a 0-d tensor and a 1-element tensor."""
    s = FORMS[form](word)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        if word & 1:
            with pytest.raises(LossExplode):
                check_status(s)
        else:
            assert check_status(s) == word
    warned = [w for w in rec if issubclass(w.category, RuntimeWarning)]
    assert len(warned) == (1 if word == 2 else 0), (word, [str(w.message) for w in rec])


def test_check_status_warns_on_every_check():
    """The non-finite bit is reported by EVERY check that sees it (a frame's check after a frame's check), not once per
    process: a run that goes non-finite in frame 40 and again in frame 41 says so twice."""
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        for _ in range(3):
            assert check_status(torch.tensor([2], dtype=torch.int32)) == 2
    assert len([w for w in rec if issubclass(w.category, RuntimeWarning)]) == 3


@pytest.mark.parametrize("words,want", [([0, 0], 0), ([1, 2], 3), ([2, 1], 3), ([2, 0, 2], 2), ([0, 1, 0], 1), ([3, 0], 3),
                                        ([2], 2), ([1, 1, 2, 0, 0], 3)])
def test_merge_status_is_a_bitwise_or(words, want):
    """ops.merge_status over the slots of one tensor, over separate one-element words, and into `out`: 1 and 2 give 3 (the
    numeric maximum, 2, would lose the reference's exit)."""
    slots = torch.tensor(words, dtype=torch.int32)
    got = ops.merge_status(slots)
    assert got.dtype == torch.int32 and tuple(got.shape) == (1,) and int(got) == want
    assert int(ops.merge_status(*[torch.tensor([w], dtype=torch.int32) for w in words])) == want
    out = torch.full((1,), 7, dtype=torch.int32)
    assert ops.merge_status(slots, out=out) is out and int(out) == want
    assert slots.tolist() == words                               # the inputs are left alone
    if len(words) > 1:                                           # `out` may be one of the inputs
        first = torch.tensor([words[0]], dtype=torch.int32)
        ops.merge_status(first, torch.tensor(words[1:], dtype=torch.int32), out=first)
        assert int(first) == want


def test_status_of_terms_is_the_definition():
    """Any term above 1e5 sets bit 0 (strictly above, compared in fp32 like the kernels), any non-finite term sets bit 1;
    +Inf sets both, -Inf and NaN only bit 1; an empty set of terms is clean."""
    def word(vals):
        return int(ops.status_of_terms(torch.tensor(vals, dtype=torch.float32).reshape(-1, 4)))
    nan, inf = float("nan"), float("inf")
    assert word([0.5, 1.0, 2.0, 0.0]) == 0
    assert word([100000.0, 0, 0, 0]) == 0 and word([100000.01, 0, 0, 0]) == 1
    assert word([0, 0, 0, 0, 0, 0, 0, 2e5]) == 1                 # any object, any term
    assert word([nan, 0, 0, 0]) == 2 and word([-inf, 0, 0, 0]) == 2 and word([-2e5, 0, 0, 0]) == 0
    assert word([inf, 0, 0, 0]) == 3
    assert word([nan, 0, 0, 0, 0, 3e5, 0, 0]) == 3
    assert int(ops.status_of_terms(torch.zeros(0, 2, 4))) == 0
    frame = torch.zeros(5, 2, 4)                                  # [n_iter, K, 4]: one bad iteration marks the frame
    frame[1, 1, 1] = 1.5e5
    frame[3, 0, 0] = nan
    assert int(ops.status_of_terms(frame)) == 3


def _or_worker(rank, world, port, q, words):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        status = torch.tensor([words[rank]], dtype=torch.int32)
        odist.allreduce_or_status_(status)
        raised = False
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            try:
                check_status(status)
            except LossExplode:
                raised = True
        q.put((rank, int(status), raised, len(rec)))
    except Exception as e:          # (reported at once: the parent must not wait out its time limit for a dead rank)
        q.put((rank, repr(e), None, None))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("words,want", [((1, 2), 3), ((2, 1), 3), ((2, 0), 2), ((0, 0), 0)])
def test_two_rank_status_is_or_reduced_gloo(words, want):
    """Two gloo ranks: one holds 1 (a term above 1e5), the other 2 (a non-finite term).  After dist.allreduce_or_status_
    BOTH see 3 and BOTH raise LossExplode -- every rank leaves together, as the reference's exit would end the job (a MAX
    reduction gives 2: both warn and train on).  Two non-exploding ranks agree on the warning; nothing hangs."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_or_worker, args=(r, 2, port, q, words)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for rank, word, raised, n_warn in res:
        assert word == want, (rank, word)
        assert raised == bool(want & 1) and n_warn == (1 if want == 2 else 0), (rank, raised, n_warn)


def test_or_collective_is_a_no_op_without_a_group():
    s = torch.tensor([2], dtype=torch.int32)
    assert odist.allreduce_or_status_(s) is s and int(s) == 2
