"""The rule of include/gp_jpeg_sync.h restated in Python, independent of csrc/jpeg_sync_core.h: positions, states, steps, the rule on an
impossible symbol, the speculative start, the rounds inside a chunk and across chunks.  On top of tests/jpeg_ref.py's marker walk (the
Huffman tables) and tests/jpeg_decode_cases.split (the stuffed scan).  For well-formed files without restart markers and without stray
markers.  analyse(file, S, C) -> namespace: n, info = (subsequences, chunks, most rounds inside a chunk, rounds across chunks), exits
(the true exit of every subsequence), begun (the blocks every subsequence begins), cuts_in_ff00, cuts_before_ff."""
from types import SimpleNamespace

import numpy as np

import jpeg_decode_cases as D
import jpeg_decode_ref as REF
import jpeg_ref as R


def _lut(table):
    """[65536]: (length, symbol) of the code at the top of 16 bits, None where none matches."""
    lut = [None] * 65536
    for (length, code), sym in table.items():
        lo = code << (16 - length)
        lut[lo:lo + (1 << (16 - length))] = [(length, sym)] * (1 << (16 - length))
    return lut


def analyse(data, S, C):
    info = R.walk(REF.strip(data))
    _, parts, _ = D.split(data)
    assert len(parts) == 1, "a file without restart markers"
    scan = parts[0]
    n = len(scan)
    data_bytes, where, i = [], [], 0                                      # the unstuffed bytes and where each lies in the scan
    while i < n:
        data_bytes.append(scan[i])
        where.append(i)
        if scan[i] == 0xff and i + 1 < n:
            assert scan[i + 1] == 0, "a stray marker"
            i += 1
        i += 1
    U = 8 * len(data_bytes)
    index = {q: j for j, q in enumerate(where)}
    bits = np.concatenate([np.unpackbits(np.array(data_bytes, dtype=np.uint8)), np.zeros(32, dtype=np.uint8)]).astype(np.int64)
    look = np.zeros(U + 1, dtype=np.int64)
    for j in range(16):
        look = look * 2 + bits[j:j + U + 1]
    look = look.tolist()                                                   # look[u]: the 16 bits from data bit u, zeros beyond the end

    def position(u):                                                       # normalised: a dropped 0x00 holds none
        return 8 * n if u >= U else 8 * where[u >> 3] + (u & 7)

    def data_bit(p):
        return U if p >= 8 * n else 8 * index[p >> 3] + (p & 7)

    is420 = info["comps"][0][1] == 2
    bpm, ny = (6, 4) if is420 else (3, 1)
    luts = {key: _lut(t) for key, t in info["dht_tables"].items()}
    dc = [luts[info["scan"][c][1]] for c in range(3)]
    ac = [luts[0x10 | info["scan"][c][2]] for c in range(3)]
    nsub, memo = -(-n // S), {}

    def exit_of(i, entry):
        """(exit(i), the blocks begun) from `entry` = (position, k, z)."""
        if (i, entry) in memo:
            return memo[i, entry]
        p, k, z = entry
        e = 8 * min((i + 1) * S, n)
        begun = 0
        if p < e:
            u = data_bit(p)
            while True:
                p = position(u)
                if p >= e:
                    break
                c = 0 if k < ny else k - ny + 1
                hit = (dc if z == 0 else ac)[c][look[u]]
                run = 0
                if hit is not None:
                    length, sym = hit
                    run, cat = (0, sym) if z == 0 else (sym >> 4, sym & 15)
                if hit is None or (z == 0 and cat > 11) or (z and (cat > 10 or (cat == 0 and run == 15 and z + 16 > 63) or (cat and z + run > 63))):
                    u, k, z = u + 1, 0, 0                                  # the rule on an impossible symbol
                    continue
                if U - u < length + cat:                                   # the symbol reaches beyond the scan: not taken
                    p = 8 * n
                    break
                u += length + cat
                if z == 0:
                    begun, z = begun + 1, 1
                elif cat == 0 and run == 15:
                    z += 16
                elif cat == 0:
                    z = 64
                else:
                    z += run + 1
                if z == 64:
                    k, z = (k + 1) % bpm, 0
        memo[i, entry] = ((p, k, z), begun)
        return memo[i, entry]

    def start(i):
        q = i * S
        return (0, 0, 0) if i == 0 else (8 * (q + (1 if scan[q - 1] == 0xff and scan[q] == 0 else 0)), 0, 0)

    true, begun, entry = [], [], (0, 0, 0)
    for i in range(nsub):
        entry, m = exit_of(i, entry)
        true.append(entry)
        begun.append(m)
    # inside the chunks
    nch = -(-nsub // C)
    ex, most = [None] * nsub, 0
    for j in range(nch):
        lanes = list(range(j * C, min((j + 1) * C, nsub)))
        ent = {s: start(s) for s in lanes}
        for s in lanes:
            ex[s] = exit_of(s, ent[s])[0]
        rounds = 0
        while True:
            differ = [s for s in lanes[1:] if ex[s - 1] != ent[s]]
            if not differ:
                break
            rounds += 1
            assert rounds <= C
            for s in differ:
                ent[s] = ex[s - 1]
            for s in differ:
                ex[s] = exit_of(s, ent[s])[0]
        most = max(most, rounds)
    # across them
    used, across = {c: start(c * C) for c in range(1, nch)}, 0
    while True:
        differ = [c for c in range(1, nch) if ex[c * C - 1] != used[c]]
        if not differ:
            break
        across += 1
        assert across <= nch
        for c in differ:
            used[c] = ex[c * C - 1]
        for c in differ:
            entry = used[c]
            for s in range(c * C, min((c + 1) * C, nsub)):
                x = exit_of(s, entry)[0]
                if x == ex[s]:
                    break
                ex[s] = entry = x
    assert ex == true, "the fixpoint is the serial decode"
    cuts = [i * S for i in range(1, nsub)]
    return SimpleNamespace(n=n, info=(nsub, nch, most, across), exits=true, begun=begun,
                           cuts_in_ff00=sum(scan[q - 1] == 0xff and scan[q] == 0 for q in cuts), cuts_before_ff=sum(scan[q] == 0xff for q in cuts))
