"""The member-sharded open of a collated BAM in pure Python, straight from its definitions and over ``bam_util.walk``: the
shares, every rank's entry e_r and the participating records in front of it (their parity is q_r), the owned couples, the
summary of a share for one candidate, and the plan with its fallbacks.  It knows nothing of segments, windows or tables."""
import struct

import bam_util as bu

DEAD, CUT = (1 << 64) - 1, (1 << 64) - 2
TAIL = 64


def boundaries(member_sizes, world):
    """S_0 .. S_W: rank r's share is the members [M r / W, M (r + 1) / W)."""
    m = len(member_sizes)
    at = [0]
    for size in member_sizes:
        at.append(at[-1] + size)
    return [at[(m * r) // world] for r in range(world + 1)]


def member_sizes(total, block):
    return [min(block, total - at) for at in range(0, total, block)] or [0]


def takes_part(entry):
    _, r, (flag, _, _) = entry
    return r is not None and bu.classify(flag) <= bu.C_SECOND


def truth(data, S):
    """From the true chain: (e_r for every rank, participating records in front of e_r, couples as (start of the first,
    start of the second) per rank, how the chain ends)."""
    H = bu.header_len(data)
    recs, end = bu.walk(data)
    chain = [t[0] for t in recs] + [end[1]]  # (the last entry: where the walk stopped)
    world = len(S) - 1
    entries, before = [H], [0]
    for r in range(1, world):
        nxt = [p for p in chain if p >= S[r]]
        entries.append(nxt[0] if nxt else None)
        before.append(sum(1 for t in recs if takes_part(t) and entries[-1] is not None and t[0] < entries[-1]))
    part = [t[0] for t in recs if takes_part(t)]
    couples = [[] for _ in range(world)]
    for c in range(len(part) // 2):
        owner = max(r for r in range(world) if entries[r] is not None and entries[r] <= part[2 * c])
        couples[owner].append((part[2 * c], part[2 * c + 1]))
    return entries, before, couples, end, len(part)


def summary(data, lo, hi, c):
    """(X, N) of the chain from lo + c through the share [lo, hi) of the inflated file ``data``."""
    T, p, n = len(data), lo + c, 0
    while p < hi:
        if p + 4 > T:
            return CUT, n
        bs = struct.unpack_from("<I", data, p)[0]
        if bs < 32:
            return DEAD, n
        if p + 36 > T:
            return CUT, n
        l_name, n_cigar, flag, l_seq = data[p + 12], struct.unpack_from("<H", data, p + 16)[0], struct.unpack_from("<H", data, p + 18)[0], struct.unpack_from("<I", data, p + 20)[0]
        if 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq <= bs and bu.classify(flag) <= bu.C_SECOND:
            n += 1
        p += 4 + bs
    return p - hi, n


def plan(data, S, seg):
    """What the definitions say the ranks do: ("ok", entries, before) or the reason of the fallback."""
    from vstrains_amd.pe import BAM_SHARD_REASONS as R

    H, T, world = bu.header_len(data), len(data), len(S) - 1
    if world > 1 and H >= S[1]:
        return R[4]
    x, n = summary(data, 0, S[1], H) if H < S[1] else (H - S[1], 0)
    entries, before = [H], [0]
    for r in range(1, world + 1):
        if x == DEAD:
            return R[6]
        if x == CUT or (r < world and S[r] + x > T):
            return R[7]
        if r == world:
            break
        if x >= min(seg, S[r + 1] - S[r]):
            return R[5]
        entries.append(S[r] + x)
        before.append(n)
        x, dn = summary(data, S[r], S[r + 1], x)
        n += dn
    if x != 0:
        return R[8]
    if n & 1:
        return R[9]
    return "ok", entries, before, n
