"""The watch sets' diff kernels alone (kernels.hip k_rows_diff_count / _scan / _emit through acl_selfcheck_rows_diff) against numpy: the records are
np.flatnonzero of the unpacked XOR, row by row, with the bit of the NEW row as `gained`.  Old rows as wide as the new ones and narrower (down to no
words at all); widths around the 16-byte loads (multiples of 4 take them, others the word loads), around a wave's step of 256 words and around the
tile of 4 096 words; one, three and 65 rows (more tiles than one block's four waves)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 4096  # kernels.hpp kDiffTileWords
WIDTHS = [0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1025, 4095, 4096, 4097, 2 * TILE + 1]
PATTERNS = ["equal", "different", "sparse", "last-bit", "beyond-old"]


@pytest.fixture(scope="module")
def engine(aclgpu_lib):
    import aclgpu
    with aclgpu.Engine("definition user {}", device=0) as e:
        yield e


def reference(old, new):
    n, width = new.shape[0], max(old.shape[1], new.shape[1])
    a, b = np.zeros((n, width), dtype=np.uint32), np.zeros((n, width), dtype=np.uint32)
    a[:, :old.shape[1]] = old
    b[:, :new.shape[1]] = new
    out = []
    for r in range(n):
        bits = np.flatnonzero(np.unpackbits((a[r] ^ b[r]).view(np.uint8), bitorder="little"))
        nb = np.unpackbits(b[r].view(np.uint8), bitorder="little")
        out.append(np.stack([np.full(bits.size, r, dtype=np.uint32), bits.astype(np.uint32), nb[bits].astype(np.uint32), np.zeros(bits.size, dtype=np.uint32)], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 4), dtype=np.uint32)


def make(rng, pattern, n, ow, nw):
    new = rng.integers(0, 1 << 32, size=(n, nw), dtype=np.uint64).astype(np.uint32)
    old = new[:, :ow].copy() if ow <= nw else np.concatenate([new, np.zeros((n, ow - nw), dtype=np.uint32)], axis=1)
    if pattern == "equal":
        new[:, ow:] = 0
    elif pattern == "different":
        old = ~old
        new[:, ow:] = 0xFFFFFFFF
    elif pattern == "sparse" and nw:  # one bit in a thousand
        new[:, ow:] = 0
        flips = (rng.random((n, max(ow, nw) * 32)) < 1e-3)
        mask = np.packbits(flips, axis=1, bitorder="little").view(np.uint32).reshape(n, -1)
        old ^= mask[:, :ow]
        new ^= mask[:, :nw]
    elif pattern == "last-bit":
        new[:, ow:] = 0
        if nw:
            new[:, nw - 1] ^= np.uint32(0x80000000)
            # (old keeps the bit as it was, or does not reach it: exactly one record per row)
    elif pattern == "beyond-old":
        pass  # (equal up to the old width, random behind it)
    return np.ascontiguousarray(old), np.ascontiguousarray(new)


@pytest.mark.parametrize("n_rows", [1, 3, 65])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_rows_diff_matches_numpy(engine, n_rows, pattern):
    rng = np.random.default_rng(1000 * n_rows + PATTERNS.index(pattern))
    cases = 0
    for nw in WIDTHS:
        olds = sorted({nw, 0, nw // 2, max(nw - 1, 0), (nw // 4) * 4 - 4 if nw >= 8 else 0})
        if n_rows == 65 and nw >= 1023:  # (65 rows: the wide ones with three old widths, and nothing wider than the largest case asked for, about 1 MB of rows)
            if nw > TILE + 1:
                continue
            olds = sorted({nw, 0, nw // 2})
        if n_rows == 65 and pattern == "different" and nw >= 1023:  # every bit a record: the big ones once each (65 x 4 097 words, about 1 MB of rows, is the largest)
            if nw > TILE + 1 or nw in (4095, 4096):
                continue
            olds = [0] if nw == TILE + 1 else [nw]
        for ow in olds:
            old, new = make(rng, pattern, n_rows, ow, nw)
            got = engine.selfcheck_rows_diff(old, new)
            want = reference(old, new)
            got4 = np.stack([got["watcher"], got["resource_id"], got["gained"], got["reserved"]], axis=1) if got.size else np.zeros((0, 4), dtype=np.uint32)
            assert got4.shape == want.shape and np.array_equal(got4, want), (n_rows, pattern, ow, nw)
            if pattern == "equal":
                assert got.size == 0
            if pattern == "last-bit" and nw:
                assert got.size == n_rows and (got["resource_id"] == nw * 32 - 1).all()
            if pattern == "beyond-old" and got.size:
                assert (got["resource_id"] >= ow * 32).all()
            cases += 1
    assert cases > 40


def test_old_rows_wider_than_new(engine):
    """(a type's id space does not shrink while a set lives, but the kernels take either order: what one array lacks reads as zero)"""
    rng = np.random.default_rng(5)
    for ow, nw in ((5, 3), (260, 255), (TILE + 3, TILE), (4, 0)):
        old = rng.integers(0, 1 << 32, size=(3, ow), dtype=np.uint64).astype(np.uint32)
        new = old[:, :nw].copy()
        got = engine.selfcheck_rows_diff(old, new)
        want = reference(old, new)
        assert got.size == want.shape[0] and np.array_equal(got["resource_id"], want[:, 1]) and not got["gained"].any() and np.array_equal(got["watcher"], want[:, 0])
