"""numpy model of the bucket copy (host/level_plan.hpp: kBktTileBytes, kBktSideBytes) and the checks of a copy read back from the
device against it (tests/test_gpu_bkt_scan.py).  The scatter is unstable, so the model fixes what does not depend on the order
inside a bucket: the buckets' slot ranges, which codes each holds, the padding, the ids, the planes as a function of the slots."""
import numpy as np

TILE = 16384
PAD = 0xffffffff
PLANES = 12
ID_OFF = PLANES * TILE // 2


def keys_of(codes):
    return codes[:, 0].astype(np.uint32) | (codes[:, 1].astype(np.uint32) << 8)


def block_layout(codes, block):
    """Per block of `block` codes: (first slot of the block, [(key, first slot in the block, count)] in key order, slots)."""
    out, first = [], 0
    for b0 in range(0, len(codes), block):
        k, cnt = np.unique(keys_of(codes[b0:b0 + block]), return_counts=True)
        padded = (cnt + 15) // 16 * 16
        start = np.concatenate([[0], np.cumsum(padded)[:-1]])
        slots = int((padded.sum() + TILE - 1) // TILE * TILE)
        out.append((first, list(zip(k.tolist(), start.tolist(), cnt.tolist())), slots))
        first += slots
    return out


def planes_of(slot_codes):
    """The 12 nibble planes and the id plane of whole tiles of slot codes [slots, 8] -> uint8 [ntiles, kBktTileBytes]."""
    nt = len(slot_codes) // TILE
    nib = np.empty((len(slot_codes), 16), np.uint8)
    nib[:, 0::2] = slot_codes & 15
    nib[:, 1::2] = slot_codes >> 4
    nib = nib.reshape(nt, TILE // 16, 2, 2, 4, 16)                # [tile][lane][dword][half: low / high nibble][byte][sub-quantizer]
    tiles = np.zeros((nt, ID_OFF + TILE // 8), np.uint8)
    for s in range(4, 16):
        plane = (nib[:, :, :, 0, :, s] | (nib[:, :, :, 1, :, s] << 4)).reshape(nt, TILE // 2)
        tiles[:, (s - 4) * (TILE // 2):(s - 3) * (TILE // 2)] = plane
    ids = keys_of(slot_codes[0::16]).astype(np.uint16).reshape(nt, TILE // 16)
    tiles[:, ID_OFF:] = ids.view(np.uint8).reshape(nt, -1)
    return tiles


def check_copy(copy, codes, block):
    """Every invariant of a copy read back (pyqadc.Index.bkt_copy) for the partition `codes`."""
    n = len(codes)
    layout = block_layout(codes, block)
    assert copy["block"] == block
    assert copy["off"].tolist() == [l[0] for l in layout] + [layout[-1][0] + layout[-1][2]]
    sc, perm = copy["codes"], copy["perm"]
    assert len(sc) == len(perm) == int(copy["off"][-1])
    real = perm != PAD
    # perm is a bijection from the real slots onto the positions, and a real slot holds its position's code
    assert np.array_equal(np.sort(perm[real]), np.arange(n, dtype=np.uint32))
    assert np.array_equal(sc[real], codes[perm[real]])
    for bi, (first, buckets, slots) in enumerate(layout):
        b0 = bi * block
        last_real = None
        used = 0
        for key, start, cnt in buckets:
            s0 = first + start
            padded = (cnt + 15) // 16 * 16
            assert real[s0:s0 + cnt].all() and not real[s0 + cnt:s0 + padded].any(), (bi, key)
            p = perm[s0:s0 + cnt]
            assert p.min() >= b0 and p.max() < b0 + block and np.all(keys_of(codes[p]) == key), (bi, key)
            assert np.all(sc[s0 + cnt:s0 + padded] == sc[s0 + cnt - 1]), (bi, key)        # padding: copies of the bucket's last code
            last_real = s0 + cnt - 1
            used = start + padded
        assert not real[first + used:first + slots].any()
        assert np.all(sc[first + used:first + slots] == sc[last_real]), bi                 # the tile's remainder: the block's last code
    # ids and planes are functions of the slot codes
    assert np.array_equal(copy["tiles"], planes_of(sc))
    assert np.all(keys_of(sc).reshape(-1, 16) == keys_of(sc[0::16])[:, None])              # one key per 16-slot group
