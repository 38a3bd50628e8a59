"""The host build of qa_idmatte_dev.h (hip.idmatte_accumulate_host, hip.idmatte_select_host: the source of qa_idmatte.hip's kernels)
against the numpy restatement of its opening comment (tests/idmatte_util.py), exactly.  No GPU."""
import itertools

import numpy as np
import pytest

from idmatte_util import EMPTY, F32, SLOTS, select_ref, table_ref
from qaray_amd import hip, host


def check(hit, keys):
    hit, keys = np.asarray(hit, bool), np.asarray(keys, np.int32)
    got = hip.idmatte_accumulate_host(hit, keys)
    ids, counts, other = table_ref(hit, keys)
    assert np.array_equal(got["ids"], ids) and np.array_equal(got["counts"], counts) and int(got["other"]) == other, (got, ids, counts, other)
    assert int(got["counts"].sum()) + int(got["other"]) == int(hit.sum())
    return got


def test_constants():
    assert (hip.QA_IDMATTE_SLOTS, hip.QA_IDMATTE_EMPTY, hip.QA_IDMATTE_NODE, hip.QA_IDMATTE_MATERIAL) == (SLOTS, EMPTY, 0, 1)
    assert EMPTY == np.iinfo(np.int32).min


def test_no_samples_and_all_misses():
    for n in (0, 1, 7):
        got = check(np.zeros(n, bool), np.arange(n))
        assert (got["ids"] == EMPTY).all() and not got["counts"].any() and int(got["other"]) == 0


def test_one_id():
    got = check(np.ones(13, bool), np.full(13, 5))
    assert got["ids"][0] == 5 and got["counts"][0] == 13 and (got["ids"][1:] == EMPTY).all()
    got = check([1, 0, 1, 0, 0, 1], [3, 9, 3, 9, 9, 3])   # the keys of misses are not read
    assert got["ids"][0] == 3 and got["counts"][0] == 3 and got["counts"][1] == 0


@pytest.mark.parametrize("distinct", [9, 12, 40])
def test_more_ids_than_slots(distinct):
    # every id once before any repeats, so the ninth arrives when the table is full; then a second round in another order
    rng = np.random.default_rng(distinct)
    first = rng.permutation(distinct) + 100
    keys = np.concatenate([first, rng.permutation(first), first[:5]])
    got = check(np.ones(len(keys), bool), keys)
    assert int(got["other"]) == (distinct - SLOTS) * 2 + max(0, 5 - SLOTS) and int(got["other"]) > 0
    assert set(got["ids"].tolist()) == set(first[:SLOTS].tolist())   # the first eight to arrive hold the table
    # with misses strewn in
    hit = rng.random(len(keys)) < 0.7
    check(hit, keys)


def test_an_id_that_arrives_when_the_table_is_full_never_enters():
    keys = list(range(8)) + [77] * 20 + [3]
    got = check(np.ones(len(keys), bool), keys)
    assert 77 not in got["ids"].tolist() and int(got["other"]) == 20
    assert got["ids"][0] == 3 and got["counts"][0] == 2   # the only slot with two samples ranks first


def test_ties_are_ordered_by_id_negative_words_among_them():
    keys = [7, -1, 4, -2, 7, -1, 4, -2, 9, 0]   # four ids with two samples each, two with one
    got = check(np.ones(len(keys), bool), keys)
    assert got["ids"][:6].tolist() == [-2, -1, 4, 7, 0, 9] and got["counts"][:6].tolist() == [2, 2, 2, 2, 1, 1]
    # every arrival order of five ids with equal counts gives one table
    for order in itertools.permutations([5, -2, 1 << 29, -1, 0]):
        got = check(np.ones(5, bool), order)
        assert got["ids"][:5].tolist() == [-2, -1, 0, 5, 1 << 29]


def test_the_ranking_network_sorts_every_pattern_of_counts():
    # a network of exchanges sorts every input if it sorts every 0/1 input: all 256 patterns of "count 1 or 2" over eight slots,
    # the ids in arrival order descending so that the ties must move too
    for pattern in range(256):
        keys = []
        for k in range(SLOTS):
            keys += [100 - k] * (2 if pattern >> k & 1 else 1)
        check(np.ones(len(keys), bool), keys)
    rng = np.random.default_rng(1)
    for _ in range(300):   # random tables, free slots and `other` included
        n = int(rng.integers(0, 60))
        check(rng.random(n) < 0.8, rng.integers(-2, int(rng.integers(1, 14)), n))


def test_the_host_hook_refuses_the_empty_id_as_a_key():
    with pytest.raises(hip.HipError):
        hip.idmatte_accumulate_host([True], [EMPTY])
    hip.idmatte_accumulate_host([False], [EMPTY])   # (not read on a miss)


def frame_of_tables(rng, npix, spp):
    ids, counts, samples = np.zeros((npix, SLOTS), np.int32), np.zeros((npix, SLOTS), np.uint32), np.zeros(npix, np.uint32)
    for q in range(npix):
        n = int(rng.integers(0, spp + 1))
        t = hip.idmatte_accumulate_host(rng.random(n) < 0.8, rng.integers(-2, 12, n))
        ids[q], counts[q], samples[q] = t["ids"], t["counts"], n
    return ids, counts, samples


def test_select():
    rng = np.random.default_rng(7)
    ids, counts, samples = frame_of_tables(rng, 200, 23)
    samples[:3] = 0
    ids[:3], counts[:3] = EMPTY, 0
    present = sorted(set(ids.ravel().tolist()) - {EMPTY})
    assert len(present) >= 10 and (samples == 0).any()
    lists = {"empty": [], "full": present, "absent": [500, -7, 12345], "one": present[:1], "some and absent": present[::3] + [999], "twice": [present[2]] * 3,
             "the empty id": [EMPTY], "most": list(range(-2, 254))}
    for name, sel in lists.items():
        got = hip.idmatte_select_host(ids, counts, samples, sel)
        want = select_ref(ids, counts, samples, sel)
        assert got.dtype == F32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    assert not hip.idmatte_select_host(ids, counts, samples, []).any() and not hip.idmatte_select_host(ids, counts, samples, [500, -7]).any()
    full = hip.idmatte_select_host(ids, counts, samples, present)
    with np.errstate(all="ignore"):
        want = np.where(samples == 0, F32(0), counts.sum(axis=1).astype(F32) / samples.astype(F32))
    assert np.array_equal(full, want.astype(F32)) and not full[samples == 0].any()
    assert np.array_equal(hip.idmatte_select_host(ids, counts, samples, [present[2]] * 3), hip.idmatte_select_host(ids, counts, samples, [present[2]]))
    # shapes: planes of a frame
    got = hip.idmatte_select_host(ids.reshape(10, 20, SLOTS), counts.reshape(10, 20, SLOTS), samples.reshape(10, 20), present[:4])
    assert got.shape == (10, 20) and np.array_equal(got.ravel(), select_ref(ids, counts, samples, present[:4]))
    with pytest.raises(ValueError):
        hip.idmatte_select_host(ids, counts, samples, list(range(257)))


def test_node_index_is_the_flatteners(tmp_path):
    from conftest import ensure_assets
    import os
    ensure_assets()
    hs = host.HostScene(os.path.join(host.SCENES_DIR, "example_project7_object.xml"))
    try:
        inst = hip.blob_table(hs.flatten(), "instances")
        # the XML's nodes in document order, children after their parent: the instance table's rows 1 ..
        assert hs.node_index("groundPlane") == 1 and inst[1]["obj_type"] == 2
        assert hs.node_index("teapot-high.obj") == 2 and inst[2]["obj_type"] == 3
        assert hs.node_index("wooddoll.obj") == 3            # the first of the four that share the name
        assert hs.node_index("suzanne.obj") == 7 and hs.node_index("sphere1") == 8 and hs.node_index("sphere2") == 9
        assert inst[8]["obj_type"] == 1 and len(inst) == 10
        with pytest.raises(KeyError):
            hs.node_index("no such node")
    finally:
        hs.close()
