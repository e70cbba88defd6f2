"""What zlib's build_tree saw, read back from a zlib stream: block type and literal/length and distance histograms of every
block (a small inflate that counts symbols instead of writing bytes), and the depth of the Huffman tree of a histogram
before gen_bitlen caps it (trees.c's pairing: smaller() on frequency, then depth)."""


class _Bits:
    def __init__(self, data):
        self.d, self.pos = bytes(data) + bytes(4), 0

    def get(self, k):  # k <= 16
        i = self.pos >> 3
        x = int.from_bytes(self.d[i:i + 4], "little") >> (self.pos & 7)
        self.pos += k
        return x & ((1 << k) - 1)


def _decoder(lengths):
    """canonical Huffman code (RFC 1951 3.2.2) -> {(length, code read MSB first): symbol}"""
    bl_count = [0] * 16
    for ln in lengths:
        if ln:
            bl_count[ln] += 1
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + bl_count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for s, ln in enumerate(lengths):
        if ln:
            table[(ln, nxt[ln])] = s
            nxt[ln] += 1
    return table


def _sym(bits, table):
    code = ln = 0
    while True:
        code = (code << 1) | bits.get(1)
        ln += 1
        if (ln, code) in table:
            return table[(ln, code)]


LEXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DEXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
BL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def blocks(stream, max_blocks=None):
    """[(btype, literal/length histogram[286], distance histogram[30], literal/length code lengths)] of a zlib stream;
    stored blocks carry None"""
    bits = _Bits(stream[2:])
    out = []
    while max_blocks is None or len(out) < max_blocks:
        final, btype = bits.get(1), bits.get(2)
        if btype == 0:
            bits.pos = (bits.pos + 7) & ~7
            n = bits.get(16)
            bits.get(16)
            bits.pos += 8 * n
            out.append((0, None, None, None))
        else:
            if btype == 1:
                llen = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
                lt = _decoder(llen)
                dt = _decoder([5] * 30)
            else:
                hlit, hdist, hclen = bits.get(5) + 257, bits.get(5) + 1, bits.get(4) + 4
                cl = [0] * 19
                for i in range(hclen):
                    cl[BL_ORDER[i]] = bits.get(3)
                ct, lens = _decoder(cl), []
                while len(lens) < hlit + hdist:
                    s = _sym(bits, ct)
                    if s < 16:
                        lens.append(s)
                    elif s == 16:
                        lens += [lens[-1]] * (3 + bits.get(2))
                    elif s == 17:
                        lens += [0] * (3 + bits.get(3))
                    else:
                        lens += [0] * (11 + bits.get(7))
                llen = lens[:hlit]
                lt, dt = _decoder(llen), _decoder(lens[hlit:])
            lf, df = [0] * 286, [0] * 30
            while True:
                s = _sym(bits, lt)
                lf[s] += 1
                if s == 256:
                    break
                if s > 256:
                    bits.get(LEXTRA[s - 257])
                    d = _sym(bits, dt)
                    df[d] += 1
                    bits.get(DEXTRA[d])
            out.append((btype, lf, df, llen))
        if final:
            break
    return out


def uncapped_depth(freqs):
    """depth of the deepest leaf of the tree trees.c's build_tree makes for a histogram, before gen_bitlen caps it at
    max_length (the overflow repair runs when this is above the limit)"""
    freq = list(freqs) + [0] * len(freqs)
    depth = [0] * len(freq)
    dad = [None] * len(freq)
    heap = [0] + [n for n, f in enumerate(freqs) if f]
    if len(heap) < 3:
        return 1

    def smaller(n, m):
        return freq[n] < freq[m] or (freq[n] == freq[m] and depth[n] <= depth[m])

    def down(k):
        v, j = heap[k], k << 1
        while j < len(heap):
            if j + 1 < len(heap) and smaller(heap[j + 1], heap[j]):
                j += 1
            if smaller(v, heap[j]):
                break
            heap[k] = heap[j]
            k, j = j, j << 1
        heap[k] = v

    for n in range((len(heap) - 1) // 2, 0, -1):
        down(n)
    node, leaves = len(freqs), [n for n, f in enumerate(freqs) if f]
    while len(heap) > 2:
        n = heap[1]
        heap[1] = heap[-1]
        heap.pop()
        down(1)
        m = heap[1]
        freq[node] = freq[n] + freq[m]
        depth[node] = max(depth[n], depth[m]) + 1
        dad[n] = dad[m] = node
        heap[1] = node
        down(1)
        node += 1

    def level(n):
        d = 0
        while dad[n] is not None:
            n, d = dad[n], d + 1
        return d
    return max(level(n) for n in leaves)


def no_match_bytes(counts, rng):
    """bytes with counts[b] copies of byte b and no 3-byte string twice, so that zlib finds no match and the literal
    histogram of the block is `counts` (plus END_BLOCK).  Stops early, a few bytes short, if every string left is taken."""
    import numpy as np
    left = np.array(counts, dtype=np.int64)
    used, out = set(), []
    while left.sum():
        cand = np.flatnonzero(left)
        for b in rng.choice(cand, size=min(64, 4 * len(cand)), p=left[cand] / left[cand].sum()):
            b = int(b)
            if len(out) < 2 or (out[-2], out[-1], b) not in used:
                break
        else:
            break
        if len(out) >= 2:
            used.add((out[-2], out[-1], b))
        out.append(b)
        left[b] -= 1
    return bytes(out)
