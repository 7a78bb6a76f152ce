"""numpy model of the bucket copy with wide octaves (host/level_plan.hpp: kBktwTileBytes) and the checks of
a copy read back from the device against it (tests/test_gpu_bktw_scan.py); tests/test_bktw_model.py runs the checks on a copy the
model builds itself, and on broken ones.  Positions from W on are cut into octaves [W 2^j, W 2^(j+1)) (the last clipped at the
partition's end); an octave whose padded slots stay within max_pad x its codes is grouped by the 20-bit key = code bytes 0, 1 and
the low nibble of byte 2 into wide tiles (11 nibble planes of sub-quantizers 5-15, a uint16 id, a byte of sub-quantizer 4); every
other range keeps narrow blocks (tests/bkt_model.py), and the narrow blocks of a wide range are empty.  As in bkt_model the
scatter's order inside a bucket is free: the model fixes the buckets' slot ranges, their codes as sets, padding, ids and planes."""
import numpy as np

import bkt_model

TILE = bkt_model.TILE
PAD = bkt_model.PAD
PLANES = 11
ID_OFF = PLANES * TILE // 2
ID4_OFF = ID_OFF + TILE // 8
TILE_BYTES = ID4_OFF + TILE // 16
SIDE_BYTES = 12 * TILE


def keys_of(codes):
    return codes[:, 0].astype(np.uint32) | (codes[:, 1].astype(np.uint32) << 8) | ((codes[:, 2].astype(np.uint32) & 15) << 16)


def octaves(n, W):
    """[(lo, hi)] of the octaves of a partition of n codes."""
    out, lo = [], W
    while W and lo < n:
        out.append((lo, min(2 * lo, n)))
        lo *= 2
    return out


def range_layout(codes, lo, hi, keyfn):
    """([(key, first slot in the range's block, count)] in key order, slots of the block: whole tiles)."""
    k, cnt = np.unique(keyfn(codes[lo:hi]), return_counts=True)
    padded = (cnt + 15) // 16 * 16
    start = np.concatenate([[0], np.cumsum(padded)[:-1]])
    return list(zip(k.tolist(), start.tolist(), cnt.tolist())), int((padded.sum() + TILE - 1) // TILE * TILE)


def wide_layout(codes, W, max_pad):
    """Per octave: (lo, hi, first slot in the wide copy, buckets, slots); slots == 0: the octave fell back to narrow blocks."""
    out, first = [], 0
    for lo, hi in octaves(len(codes), W):
        buckets, slots = range_layout(codes, lo, hi, keys_of)
        if slots > max_pad * (hi - lo):
            buckets, slots = [], 0
        out.append((lo, hi, first, buckets, slots))
        first += slots
    return out


def narrow_layout(codes, block, wide):
    """Per narrow block: (lo, hi, first slot in the narrow copy, buckets, slots); a block inside a wide octave: no slots."""
    out, first = [], 0
    for lo in range(0, len(codes), block):
        hi = min(lo + block, len(codes))
        covered = any(slots and olo <= lo < ohi for olo, ohi, _, _, slots in wide)
        buckets, slots = ([], 0) if covered else range_layout(codes, lo, hi, bkt_model.keys_of)
        out.append((lo, hi, first, buckets, slots))
        first += slots
    return out


def planes_of(slot_codes):
    """The wide tiles of whole tiles of slot codes [slots, 8] -> uint8 [ntiles, TILE_BYTES]."""
    nt = len(slot_codes) // TILE
    nib = np.empty((len(slot_codes), 16), np.uint8)
    nib[:, 0::2] = slot_codes & 15
    nib[:, 1::2] = slot_codes >> 4
    grp = nib.reshape(nt, TILE // 16, 2, 2, 4, 16)               # [tile][lane][dword][half: low / high nibble][byte][sub-quantizer]
    tiles = np.zeros((nt, TILE_BYTES), np.uint8)
    for s in range(5, 16):
        plane = (grp[:, :, :, 0, :, s] | (grp[:, :, :, 1, :, s] << 4)).reshape(nt, TILE // 2)
        tiles[:, (s - 5) * (TILE // 2):(s - 4) * (TILE // 2)] = plane
    ids = bkt_model.keys_of(slot_codes[0::16]).astype(np.uint16).reshape(nt, TILE // 16)
    tiles[:, ID_OFF:ID4_OFF] = ids.view(np.uint8).reshape(nt, -1)
    tiles[:, ID4_OFF:] = nib[0::16, 4].reshape(nt, TILE // 16)
    return tiles


def model_copy(codes, layout, planesfn, block):
    """A copy as the device could have built it (the stable one: bucket order = position order) -> the dict of Index.bkt(w)_copy."""
    total = layout[-1][2] + layout[-1][4] if layout else 0
    sc = np.zeros((total, 8), np.uint8)
    perm = np.full(total, PAD, np.uint32)
    for lo, hi, first, buckets, slots in layout:
        if not slots:
            continue
        keyfn = keys_of if planesfn is planes_of else bkt_model.keys_of
        kk = keyfn(codes[lo:hi])
        last = None
        for key, start, cnt in buckets:
            pos = lo + np.nonzero(kk == key)[0]
            s0 = first + start
            sc[s0:s0 + cnt] = codes[pos]
            perm[s0:s0 + cnt] = pos
            sc[s0 + cnt:s0 + (cnt + 15) // 16 * 16] = codes[pos[-1]]
            last, used = codes[pos[-1]], start + (cnt + 15) // 16 * 16
        sc[first + used:first + slots] = last
    return {"block": block, "off": np.array([l[2] for l in layout] + [total], np.uint64), "tiles": planesfn(sc), "codes": sc, "perm": perm}


def check_layout(copy, codes, layout, keyfn, planesfn):
    """The invariants of one copy (wide or narrow) whose blocks are `layout`: every code of a stored range once in a real slot of
    its own block, one key per 16-slot group, padding copies inside their own bucket, planes and ids functions of the side array."""
    sc, perm = copy["codes"], copy["perm"]
    total = layout[-1][2] + layout[-1][4] if layout else 0
    assert copy["off"].tolist() == [l[2] for l in layout] + [total]
    assert len(sc) == len(perm) == total
    real = perm != PAD
    stored = np.concatenate([np.arange(lo, hi, dtype=np.uint32) for lo, hi, _, _, slots in layout if slots] + [np.zeros(0, np.uint32)])
    assert np.array_equal(np.sort(perm[real]), stored)           # a bijection from the real slots onto the stored positions
    assert np.array_equal(sc[real], codes[perm[real]])
    for lo, hi, first, buckets, slots in layout:
        if not slots:
            continue
        used, last_real = 0, None
        for key, start, cnt in buckets:
            s0, padded = first + start, (cnt + 15) // 16 * 16
            assert real[s0:s0 + cnt].all() and not real[s0 + cnt:s0 + padded].any(), (lo, key)
            p = perm[s0:s0 + cnt]
            assert p.min() >= lo and p.max() < hi and np.all(keyfn(codes[p]) == key), (lo, key)
            assert np.all(sc[s0 + cnt:s0 + padded] == sc[s0 + cnt - 1]), (lo, key)     # padding: copies of the bucket's last code
            last_real, used = s0 + cnt - 1, start + padded
        assert not real[first + used:first + slots].any()
        assert np.all(sc[first + used:first + slots] == sc[last_real]), lo              # the tile's remainder: the block's last code
    assert np.array_equal(copy["tiles"], planesfn(sc))
    assert np.all(keyfn(sc).reshape(-1, 16) == keyfn(sc[0::16])[:, None])               # one key per 16-slot group


def check_copies(wide_copy, narrow_copy, codes, W, block, max_pad):
    """Both copies of a partition against the model -> (the wide layout, the narrow layout).  A partition without a wide octave
    has no wide copy (None); one whose narrow blocks are all covered has no narrow copy."""
    wide = wide_layout(codes, W, max_pad)
    narrow = narrow_layout(codes, block, wide)
    if any(l[4] for l in wide):
        assert wide_copy is not None and wide_copy["block"] == W
        check_layout(wide_copy, codes, wide, keys_of, planes_of)
    else:
        assert wide_copy is None
    if any(l[4] for l in narrow):
        assert narrow_copy is not None and narrow_copy["block"] == block
        check_layout(narrow_copy, codes, narrow, bkt_model.keys_of, bkt_model.planes_of)
    else:
        assert narrow_copy is None
    # together: every code of the partition once
    every = np.concatenate([c["perm"][c["perm"] != PAD] for c in (wide_copy, narrow_copy) if c is not None])
    assert np.array_equal(np.sort(every), np.arange(len(codes), dtype=np.uint32))
    return wide, narrow
