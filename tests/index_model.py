"""The model and the sequence generator of the lifecycle tests (tests/test_index_model_host.py, tests/test_gpu_adc_lifecycle.py,
tests/test_gpu_index_lifecycle.py): what an index holds after any sequence of add_vectors / reserve / remove_labels / add_partitions
calls, in numpy, and deterministic sequences of such calls that are built to reach the states one call leaves for the next.

Pure numpy, no GPU.  The model is made of the helpers the single-feature tests use — group and append (test_gpu_adc_add.py),
model_remove (test_gpu_adc_remove.py) — over a pool of vectors that is encoded once per shape.  A sequence depends on the pool
through the coarse assignment alone (which partition a row goes to), so the CPU test and the GPU tests generate the same one.

Sizes: K = 4 partitions and a pool of 24 000 vectors, about 6000 per partition, so that a partition can hold more than
kRemoveTile = 4096 rows: the smallest size at which the compaction has a second tile and a write that lags a tile."""
import numpy as np

import adc_compose as ac
import adc_filter_compose as fc
from helpers import float_tables
from test_gpu_adc_add import TILE as ADD_TILE
from test_gpu_adc_add import Quantizers, append, group
from test_gpu_adc_remove import T as REMOVE_TILE
from test_gpu_adc_remove import model_remove

K = 4
POOL = 24000
NQ, MA = 4, 3
BIG = REMOVE_TILE + 600                                                          # rows per partition of the large phase

# (nsq, bits, dim) and the seeds of the float-ADC walks; OPQ on one 8-bit and one 16-bit shape
ADC_CASES = [((4, 8, 16), 0), ((8, 8, 64), 0), ((8, 8, 64), 1), ((16, 8, 32), 0), ((2, 16, 16), 0), ((2, 16, 16), 1), ((8, 16, 16), 0)]
ADC_OPQ = {(8, 8, 64), (2, 16, 16)}
# (M, 4, dim), the starting point and the seed of the 4-bit walks: the long ones and the short ones that run under every scan path
INDEX4_CASES = [((16, 4, 32), "own", 0), ((16, 4, 32), "fresh", 1), ((32, 4, 64), "own_after_remove", 0), ((32, 4, 64), "fresh", 1)]
INDEX4_SHORT_CASES = [((16, 4, 32), "fresh", 2), ((32, 4, 64), "own_after_remove", 2)]

KINDS = ("adc", "index4", "index4_short")
STARTS = ("fresh", "own", "own_after_remove")
KEEPS = (0.5, 0.01)                                                              # finalize's keep at the 4-bit walks' check steps, in turn
ADDS = ("add", "add_device", "refill_in_place", "overflow")
REMOVES = ("remove", "remove_device", "empty_partition", "empty_index", "remove_found")
MUTATIONS = ADDS + REMOVES + ("remove_nothing", "reserve_more", "reserve_less", "add_partitions", "start_partitions")


def case_id(case):
    return "-".join(["%dx%d-d%d" % case[0]] + [str(x) for x in case[1:]])


# ---- the pool ----------------------------------------------------------------------------------------------------------------

_quantizers = {}


def quantizers(shape):
    """One shape's codebooks, K coarse centroids, a rotation and POOL clustered vectors (test_gpu_adc_add.Quantizers; Quantizers4 for
    4-bit sub-quantizers).  Building it runs nothing on a GPU."""
    if shape not in _quantizers:
        nsq, bits, dim = shape
        if bits == 4:
            from test_gpu_index_add import Quantizers4
            _quantizers[shape] = Quantizers4(nsq, dim, K=K, n=POOL, seed=40)
        else:
            _quantizers[shape] = Quantizers(nsq, bits, dim, K=K, n=POOL, seed=40)
    return _quantizers[shape]


def far_centroid(q):
    """a fifth coarse centroid that no pool vector is nearest to: the partition that add_partitions appends during a float-ADC walk
    gets rows from that call alone"""
    return np.full((1, q.dim), 9.0, np.float32)


def queries(q):
    """NQ query vectors: one near each of three coarse centroids and one at the far centroid, so that every partition is probed"""
    rng = np.random.default_rng(4100 + q.nsq + q.bits)
    at = np.concatenate([q.coarse[:NQ - 1], far_centroid(q)])
    return (at + 0.5 * rng.normal(size=(NQ, q.dim))).astype(np.float32)


def coarse_of(q, partitions):
    return q.coarse if partitions <= K else np.concatenate([q.coarse, far_centroid(q)])


_host_assign, _host_pools = {}, {}


def host_assign(po, shape):
    """assign [POOL] from the CPU oracle's find_k_neighbors(k = 1): what the sequences of the CPU test are generated from.  The GPU
    tests hold the library's encoders to it before they walk the same sequences."""
    if shape not in _host_assign:
        q = quantizers(shape)
        a = ac.assign(po, q.vectors, coarse_of(q, K + 1), 1)[:, 0].copy()
        assert a.max() < K, "a pool vector is nearest to the far centroid"
        _host_assign[shape] = a
    return _host_assign[shape]


def host_pool(po, shape, opq=False):
    """(assign [POOL], codes [POOL][...]) from the CPU oracle: host_assign, and the codes of adc_compose.encode (8-bit) or
    po.pq_encode (4-bit sub-quantizers).  The oracle's 16-bit encoder goes through a 24 000 x 65 536 distance matrix per
    sub-quantizer, too much for a quick CPU test: there the codes are random stand-ins — the CPU test uses codes only to look
    random tables up, which tells real codes and random ones apart in nothing."""
    key = (shape, opq)
    if key not in _host_pools:
        nsq, bits, dim = shape
        q = quantizers(shape)
        a = host_assign(po, shape)
        rotation = q.rotation if opq else None
        if bits == 8:
            a8, codes = ac.encode(po, q.codebooks, q.vectors, q.coarse, rotation)
            assert np.array_equal(a8, a)
        elif bits == 4:
            resid = (q.vectors - q.coarse[a]).astype(np.float32)
            codes = po.pq_encode(q.codebooks, resid, rotation, form=1, sum_mode=1)
        else:
            codes = fc.rand_codes(np.random.default_rng(16 + nsq), (nsq, bits), POOL)
        _host_pools[key] = (a, codes)
    return _host_pools[key]


def extra_partition(shape, seed, labels):
    """the (codes, labels) of the partition a float-ADC walk appends with add_partitions: random codes"""
    nsq, bits, _ = shape
    return fc.rand_codes(np.random.default_rng(7000 + seed), (nsq, bits), len(labels)), np.asarray(labels, np.uint32)


# ---- the queries of the 4-bit walks' check steps ----------------------------------------------------------------------------

def index4_inputs(shape, seed):
    """(assign [NQ][MA], tables [NQ][MA][M*16]) of a 4-bit walk's query_scan calls: three distinct probes per query"""
    M = shape[0]
    rng = np.random.default_rng(500 + M + seed)
    assign = np.stack([rng.permutation(K)[:MA] for _ in range(NQ)]).astype(np.int32)
    return assign, float_tables(rng, NQ, MA, M)


def start_size(n, keep):
    """the codes of a partition of n that finalize(keep) pre-scans: min(max(1, unsigned(float(n) * keep)), n), none of none"""
    return min(max(1, int(np.float32(n) * np.float32(keep))), n) if n else 0


def index4_keep(sizes, assign, ordinal, R=100):
    """finalize's keep at check number `ordinal`: 0.5 and 0.01 in turn, but 0.5 wherever the starts of a query's probes would not
    fill a heap of R at 0.01 — scanner_4 answers such a query with status 1 and no heap, and nothing would be compared"""
    def fills(keep):
        return all(sum(start_size(sizes[p], keep) for p in probes) >= R for probes in assign)
    keep = KEEPS[ordinal % 2]
    return keep if fills(keep) else KEEPS[0]


def found_filter(held):
    """the allow set under which a 4-bit walk's view searches for the keys remove_found takes: 70 % of the labels held"""
    return np.random.default_rng(len(held) + 1).permutation(held)[:len(held) * 7 // 10]


def with_keys_of(sequence, donor):
    """the sequence with the key set of its n-th set_filter step replaced by that of the donor's n-th: the second of two walks that
    share their AdcFilter objects"""
    given = [st for st in donor if st["op"] == "set_filter" and st["mode"] is not None]
    out, n = [], 0
    for st in sequence:
        if st["op"] == "set_filter" and st["mode"] is not None:
            assert given[n]["mode"] == st["mode"]
            st = dict(st, keys=given[n]["keys"])
            n += 1
        out.append(st)
    return out


# ---- the model ---------------------------------------------------------------------------------------------------------------

class Model:
    """[(codes, labels)] per partition.  assign [n], codes [n][...]: the pool, every vector encoded on its own"""

    def __init__(self, assign, codes, partitions=K):
        self.assign, self.codes, self.K = np.asarray(assign), codes, partitions
        self.parts = []

    def reserve(self):
        """reserve and the first add_vectors create the K partitions of the coarse quantizer"""
        if not self.parts:
            self.parts = [(self.codes[:0], np.zeros(0, np.uint32)) for _ in range(self.K)]

    def add(self, rows, labels_offset):
        """add_vectors(vectors[rows], labels_offset): vector i of the call goes behind its partition's rows with label labels_offset + i"""
        self.reserve()
        rows = np.asarray(rows, np.int64)
        self.parts = append(self.parts, group(self.assign[rows], self.codes[rows], len(self.parts), labels_offset))

    def remove(self, labels):
        self.parts, gone = model_remove(self.parts, labels)
        return gone

    def add_partitions(self, parts):
        self.parts = self.parts + [(np.asarray(c), np.asarray(l, np.uint32)) for c, l in parts]

    def start(self, rows, labels_offset):
        """the partitions add_partitions is given at an "own" start: the grouping of the pool's rows"""
        rows = np.asarray(rows, np.int64)
        return group(self.assign[rows], self.codes[rows], self.K, labels_offset)

    def sizes(self):
        return [len(c) for c, _ in self.parts]

    def labels(self):
        return np.concatenate([l for _, l in self.parts]) if self.parts else np.zeros(0, np.uint32)


# ---- the sequences -----------------------------------------------------------------------------------------------------------

class Profile:
    """what a sequence is generated for.  kind "adc": a float-ADC walk with filters, finishes and one add_partitions; "index4": the
    4-bit index's long walk; "index4_short": its walk of a few steps for the query checks under every scan path.  start: "fresh"
    (add_vectors from nothing), "own" (add_partitions of the pool's first third, each partition an allocation of its own) or
    "own_after_remove" (the same, shortened by a removal before the first add_vectors).  shape (nsq, bits, dim): rows of 8 bytes
    ask for odd row counts."""

    def __init__(self, kind, assign, start, shape):
        assert kind in KINDS and start in STARTS and (kind != "adc" or start == "fresh")
        self.kind, self.assign, self.start, self.shape = kind, np.asarray(assign), start, tuple(shape)
        self.row_bytes = shape[0] * shape[1] // 8
        self.filters = kind == "adc"
        self.short = kind == "index4_short"


def required(profile):
    """the coverage conditions a sequence of this profile guarantees"""
    if profile.short:
        need = ["refill_directly_after_remove", "overflow", "add_count_on_the_tile_edge"]
    else:
        need = ["refill_directly_after_remove", "overflow", "empty_partition_then_an_add_that_reaches_it", "empty_index_then_add",
                "remove_nothing", "reserve_less", "reserve_after_a_removal", "above_below_above_the_remove_tile", "add_count_on_the_tile_edge",
                "a_label_held_by_two_partitions"]
    if profile.row_bytes == 8:
        need += ["odd_row_count_left_by_a_remove", "odd_row_count_left_by_an_add"]
    if profile.filters:
        need += ["check_after_a_mutation_without_filter", "check_after_a_mutation_under_exclude", "check_after_a_mutation_under_allow",
                 "check_after_a_mutation_with_finish_0", "check_after_a_mutation_with_finish_1", "add_partitions_after_a_relocation"]
    return need


class _Walk:
    def __init__(self, seed, profile):
        self.pf = profile
        self.rng = np.random.default_rng([seed, KINDS.index(profile.kind), STARTS.index(profile.start)] + list(profile.shape))
        self.assign = profile.assign
        n = len(self.assign)
        self.m = Model(self.assign, np.arange(n).reshape(n, 1))                  # (the codes stand for the pool's rows)
        self.unused = np.ones(n, bool)
        self.next_label = int(self.rng.integers(1, 50))                          # (label 0, the key of a heap's sentinels, is never held)
        self.cap_bound = np.zeros(K, np.int64)                                   # no partition's capacity exceeds it
        self.freed = np.zeros(K, np.int64)
        self.out = []

    # -- bookkeeping
    def sizes(self):
        self.m.reserve()
        return np.array(self.m.sizes()[:K], np.int64)

    def fresh_labels(self, count):
        first = self.next_label
        self.next_label += count + int(self.rng.integers(1, 500))
        return first

    def pick(self, counts):
        """rows of the pool that the index does not hold, counts[p] of them assigned to partition p, in input order"""
        rows = []
        for p in range(K):
            free = np.flatnonzero(self.unused & (self.assign == p))
            assert len(free) >= counts[p], "the pool has %d free rows of partition %d, %d are asked for" % (len(free), p, counts[p])
            rows.append(self.rng.choice(free, int(counts[p]), replace=False))
        return np.sort(np.concatenate(rows))

    def odd(self, sizes):
        return self.pf.row_bytes != 8 or bool((np.asarray(sizes) % 2 == 1).any())

    def add(self, rows, op="add", fits=None, labels_offset=None):
        rows = np.asarray(rows, np.int64)
        count = np.bincount(self.assign[rows], minlength=K)
        first = self.fresh_labels(len(rows)) if labels_offset is None else labels_offset
        total = self.sizes() + count
        self.m.add(rows, first)
        self.unused[rows] = False
        self.cap_bound = np.maximum(self.cap_bound, total + (total + 1) // 2 + 16)   # (host/adc_append_plan.hpp: 1.5 x, a 16-byte word)
        self.out.append(dict(op=op, rows=rows, labels_offset=first, fits=fits))

    def remove(self, labels, op="remove", **more):
        labels = self.rng.permutation(np.asarray(labels, np.uint32))
        before = self.sizes()
        gone = self.m.remove(labels)
        self.freed = before - self.sizes()
        self.out.append(dict(op=op, labels=labels, gone=gone, **more))

    def some_labels(self, fraction):
        """a random fraction of every partition's labels"""
        return np.concatenate([l[self.rng.random(len(l)) < fraction] for _, l in self.m.parts[:K]])

    def emit(self, op, **args):
        self.out.append(dict(op=op, **args))

    def check(self, **args):
        self.emit("check", **args)

    def set_filter(self, mode):
        """a filter over 30 % of the labels the index holds and every other label of the next 30 000"""
        if not self.pf.filters:
            return
        if mode is None:
            self.emit("set_filter", mode=None, keys=None)
            return
        held = self.m.labels()
        keys = np.concatenate([held[self.rng.random(len(held)) < 0.3], np.arange(self.next_label, self.next_label + 30000, 2)])
        self.emit("set_filter", mode=mode, keys=self.rng.permutation(keys).astype(np.uint32))

    def set_finish(self, mode):
        if self.pf.filters:
            self.emit("set_finish", mode=mode)

    # -- the parts of a sequence
    def begin(self):
        edge = ADD_TILE + int(self.rng.integers(-1, 2))                          # 1023, 1024 or 1025 vectors: one tile of the dispatch, and its edges
        if self.pf.start == "fresh":
            rows = np.sort(self.rng.choice(len(self.assign), edge, replace=False))
            # capacities reserved before the index has labels; full partitions, so that one more row would relocate
            self.emit("reserve_more", capacities=np.bincount(self.assign[rows], minlength=K))
            self.cap_bound = np.bincount(self.assign[rows], minlength=K) + 16
            self.add(rows, fits=True)
            return
        third = np.arange(len(self.assign) // 3)
        first = self.fresh_labels(len(third))
        self.m.add_partitions(self.m.start(third, first))
        self.unused[third] = False
        self.cap_bound = self.sizes() + 16
        self.emit("start_partitions", rows=third, labels_offset=first)
        if self.pf.start == "own_after_remove":
            self.remove(self.some_labels(0.25))
        # the first add_vectors moves the allocations add_partitions made into the arena
        self.add(self.pick(np.bincount(self.rng.integers(0, K, edge), minlength=K)), fits="moves")

    def small_phase(self):
        """hundreds to a few thousand rows per partition"""
        # one label held by two rows in two partitions: a one-vector add_vectors whose labels_offset is a label of another partition
        row = int(self.pick(np.eye(K, dtype=np.int64)[0])[0])
        twice = int(self.m.parts[1][1][len(self.m.parts[1][1]) // 2])
        self.add([row], labels_offset=twice)
        self.check()
        labels = np.concatenate([[twice], self.some_labels(1 / 3)]).astype(np.uint32)
        if not self.odd([len(c) for c, _ in model_remove(self.m.parts[:K], labels)[0]]):
            labels = labels[:-1]                                                 # one row more stays: its partition's count is odd
        assert self.odd([len(c) for c, _ in model_remove(self.m.parts[:K], labels)[0]])
        self.remove(labels)
        # fewer new rows than were removed from each partition: the freed room takes them
        count = np.maximum(self.freed - 1, 1)
        if not self.odd(self.sizes() + count):
            count[int(np.argmax(count))] -= 1
        assert (count >= 1).all() and (count <= self.freed).all() and self.odd(self.sizes() + count)
        self.add(self.pick(count), "refill_in_place", fits=True)
        self.check()
        if self.pf.short:
            return
        self.set_filter("exclude")
        # at least as many new rows as a partition holds, and more than any capacity the rule may have rounded to
        self.add(self.pick(np.maximum(self.sizes(), self.cap_bound - self.sizes() + 1)), "overflow", fits="moves")
        self.check()
        p = int(self.rng.integers(0, K))
        self.remove(self.m.parts[p][1], "empty_partition", partition=p)
        self.check()
        self.add(self.pick(np.full(K, 40) + self.rng.integers(0, 20, K)), "add_device")
        self.emit("remove_nothing", labels=np.arange(self.next_label + 40000, self.next_label + 40007, dtype=np.uint32))
        self.emit("reserve_less", capacities=np.ones(K, np.int64))
        self.check()
        self.remove(self.some_labels(0.2), "remove_device")
        room = self.sizes() + 300                                                # a reserve after a removal, and adds into its room
        self.emit("reserve_more", capacities=room)
        self.cap_bound = np.maximum(self.cap_bound, room + 16)
        self.add(self.pick(np.full(K, 200) + self.rng.integers(0, 50, K)), fits=True)
        self.set_filter(None)
        self.check()
        self.remove(self.m.labels(), "empty_index")
        self.unused[:] = True                                                    # the index holds nothing: every row of the pool is free again
        self.check()

    def large_phase(self):
        """every partition above kRemoveTile rows, below it, and above it again"""
        count = np.full(K, BIG) + self.rng.integers(0, 30, K)
        if (count > self.cap_bound).all():                                       # (the capacities outlive the rows: an "own" start has grown them already)
            self.add(self.pick(count), "overflow", fits="moves")
        else:
            self.add(self.pick(count))
        self.set_finish(1)
        self.set_filter("allow")
        self.check()
        self.remove(self.some_labels(0.2), "remove_device")                      # BIG * 0.8 < kRemoveTile
        assert (self.sizes() < REMOVE_TILE).all()
        self.check(view=True)
        self.set_filter("exclude")
        if self.pf.filters:
            first = self.fresh_labels(700)
            labels = self.rng.permutation(np.arange(first, first + 700, dtype=np.uint32))
            self.m.add_partitions([(np.full((700, 1), -1), labels)])
            self.emit("add_partitions", labels=labels, seed=int(self.rng.integers(0, 1000)))
            self.check(deep=True)
        self.add(self.pick(REMOVE_TILE + 1 + self.rng.integers(0, 50, K) - self.sizes()))
        self.set_finish(0)
        self.check()
        self.set_filter(None)
        # directly after a check: on the 4-bit index neither call ends what finalize set up
        self.emit("remove_nothing", labels=np.arange(self.next_label + 40000, self.next_label + 40003, dtype=np.uint32))
        self.emit("reserve_less", capacities=np.ones(K, np.int64))
        self.check()

    def end(self):
        self.emit("remove_found")                                                # the keys a search returns, known when it runs
        self.check()

    def run(self):
        self.begin()
        self.small_phase()
        if self.pf.short:
            self.add(self.pick(np.maximum(self.sizes(), self.cap_bound - self.sizes() + 1)), "overflow", fits="moves")
            self.check(view=True)
        else:
            self.large_phase()
        self.end()
        return self.out


def steps(seed, profile):
    """-> [dict(op=..., ...)]: the sequence of the seed for the profile.  The coverage conditions of required(profile) hold, or the
    call fails."""
    out = _Walk(seed, profile).run()
    got = coverage(out, profile)
    missing = [name for name in required(profile) if not got[name]]
    assert not missing, "the sequence of seed %d misses %s" % (seed, missing)
    return out


def same_steps(a, b):
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x.keys() != y.keys():
            return False
        for k in x:
            if isinstance(x[k], np.ndarray) or isinstance(y[k], np.ndarray):
                if not (isinstance(x[k], np.ndarray) and isinstance(y[k], np.ndarray) and x[k].dtype == y[k].dtype and np.array_equal(x[k], y[k])):
                    return False
            elif x[k] != y[k]:
                return False
    return True


def apply(model, step, shape=None):
    """the step's effect on the model; -> the rows a removal took, or None.  (remove_found is applied by its caller, which knows
    the keys.)"""
    op = step["op"]
    if op in ADDS:
        model.add(step["rows"], step["labels_offset"])
    elif op in ("remove", "remove_device", "empty_partition", "empty_index"):
        return model.remove(step["labels"])
    elif op == "remove_nothing":
        assert model.remove(step["labels"]) == 0
    elif op in ("reserve_more", "reserve_less"):
        model.reserve()
    elif op == "start_partitions":
        model.add_partitions(model.start(step["rows"], step["labels_offset"]))
    elif op == "add_partitions":
        codes, labels = extra_partition(shape, step["seed"], step["labels"]) if shape else (np.full((len(step["labels"]), 1), -1), step["labels"])
        model.add_partitions([(codes, labels)])
    return None


def coverage(sequence, profile):
    """name -> bool for every coverage condition, found by replaying the sequence's own arguments on a model of row numbers"""
    n = len(profile.assign)
    m = Model(profile.assign, np.arange(n).reshape(n, 1))
    names = required(Profile("adc", profile.assign, "fresh", (8, 8, 0))) + required(Profile("index4", profile.assign, "fresh", (16, 4, 0)))
    got = {name: False for name in names}
    emptied, index_emptied, relocated, mutated = set(), False, False, False
    life = [[] for _ in range(K)]                                                # per partition: above / below kRemoveTile, as it changed
    mode, finish = None, 0
    for i, st in enumerate(sequence):
        op = st["op"]
        if op == "remove_found":
            break                                                                # (the last mutation: its keys are known when it runs)
        before = np.array((m.sizes() + [0] * K)[:K])
        apply(m, st)
        after = np.array((m.sizes() + [0] * K)[:K])
        mutated = mutated or op in MUTATIONS
        for p in range(K):
            side = "above" if after[p] > REMOVE_TILE else "below" if after[p] < REMOVE_TILE else None
            if side and (not life[p] or life[p][-1] != side):
                life[p].append(side)
        if op in ADDS:
            count = after - before
            got["refill_directly_after_remove"] |= op == "refill_in_place" and sequence[i - 1]["op"] in ("remove", "remove_device") \
                and bool((count <= np.maximum(prev_freed, 0)).all())
            got["overflow"] |= op == "overflow" and bool((count >= before).all())
            got["empty_partition_then_an_add_that_reaches_it"] |= any(count[p] > 0 for p in emptied)
            got["empty_index_then_add"] |= index_emptied
            got["add_count_on_the_tile_edge"] |= len(st["rows"]) in (ADD_TILE - 1, ADD_TILE, ADD_TILE + 1)
            got["odd_row_count_left_by_an_add"] |= bool(((after % 2 == 1) & (count > 0)).any())
            relocated = relocated or st["fits"] == "moves"
            emptied, index_emptied = set(), False
            labels = m.labels()
            got["a_label_held_by_two_partitions"] |= len(np.unique(labels)) < len(labels)
        elif op in REMOVES:
            got["odd_row_count_left_by_a_remove"] |= bool(((after % 2 == 1) & (after < before)).any())
            if op == "empty_partition":
                assert after[st["partition"]] == 0 < before[st["partition"]]
                emptied.add(st["partition"])
            if op == "empty_index":
                assert after.sum() == 0 < before.sum()
                index_emptied = True
        elif op == "remove_nothing":
            got["remove_nothing"] = True
        elif op == "reserve_less":
            got["reserve_less"] |= bool((np.asarray(st["capacities"]) <= before).all()) and before.sum() > 0
        elif op == "reserve_more":
            got["reserve_after_a_removal"] |= i > 0 and sequence[i - 1]["op"] in REMOVES and bool((np.asarray(st["capacities"]) > before).all())
        elif op == "add_partitions":
            got["add_partitions_after_a_relocation"] |= relocated
        elif op == "set_filter":
            mode = st["mode"]
        elif op == "set_finish":
            finish = st["mode"]
        elif op == "check" and mutated:
            got["check_after_a_mutation_" + ("without_filter" if mode is None else "under_" + mode)] = True
            got["check_after_a_mutation_with_finish_%d" % finish] = True
            mutated = False
        prev_freed = before - after
    got["above_below_above_the_remove_tile"] = any("above,below,above" in ",".join(l) for l in life)
    return got


def brute_force(sequence, assign, codes, found=None, shape=None):
    """The partitions after the whole sequence, computed without the model's steps: every (pool row, label) pair in insertion order,
    the removed labels struck out, grouped stably by assignment at the end.  found: the keys of remove_found."""
    rows, labels = np.zeros(0, np.int64), np.zeros(0, np.uint32)
    extra = []
    for st in sequence:
        op = st["op"]
        if op in ADDS or op == "start_partitions":
            rows = np.concatenate([rows, np.asarray(st["rows"], np.int64)])
            labels = np.concatenate([labels, (np.arange(len(st["rows"])) + st["labels_offset"]).astype(np.uint32)])
        elif op in REMOVES or op == "remove_nothing":
            gone = np.asarray(found if op == "remove_found" else st["labels"], np.uint32)
            keep = ~np.isin(labels, gone)
            rows, labels = rows[keep], labels[keep]
            extra = [(c[~np.isin(l, gone)], l[~np.isin(l, gone)]) for c, l in extra]
        elif op == "add_partitions":
            extra.append(extra_partition(shape, st["seed"], st["labels"]))
    order = np.argsort(assign[rows], kind="stable")
    a = assign[rows][order]
    parts = [(codes[rows[order][a == p]], labels[order][a == p]) for p in range(K)]
    return parts + extra
