"""The constructed windows the tests of the pairing by read name share (tests/pair_names_model.py is the model): the smallest
shapes at which the kernels of csrc/vs_pair_names.hip can go wrong.  A case is (name, window 1, window 2, options for
``pe.fastq_join``: ``table``, ``name_bits``); both windows end their files unless the test says otherwise."""
from interleaved_model import record

import pair_names_model as pm


def mates_files(n: int, style: int = 0):
    """two files of n mates each, the names written in turn as /1 /2, with a comment, and bare"""
    h0, h1 = [], []
    for k in range(n):
        kind = (k + style) % 3
        if kind == 0:
            h0.append(b"@r%d/1" % k), h1.append(b"@r%d/2" % k)
        elif kind == 1:
            h0.append(b"@r%d 1:N:0:AC" % k), h1.append(b"@r%d 2:N:0:AC" % k)
        else:
            h0.append(b"@r%d" % k), h1.append(b"@r%d" % k)
    return h0, h1


def text(headers, shift: int = 0) -> bytes:
    return b"".join(record(h, k + shift) for k, h in enumerate(headers))


EDGE_SIZES = (63, 64, 65, 255, 256, 257)  # wavefront and workgroup edges of the compaction


def colliding_keys(table: int, slot: int, n: int):
    """n names whose hash lands on `slot` of a table of `table` slots"""
    out, k = [], 0
    while len(out) < n:
        name = b"@w%d" % k
        if pm.pn_hash(name) & (table - 1) == slot:
            out.append(name)
        k += 1
    return out


def aligned_headers():
    """two files in which a header line starts at every byte offset mod 16: sequence lines of every length 1..16 in front"""
    h0, h1 = mates_files(96)
    t0 = b"".join(h + b"\n" + b"A" * (1 + k % 16) + b"\n+\n" + b"I" * (1 + k % 16) + b"\n" for k, h in enumerate(h0))
    t1 = b"".join(h + b"\n" + b"C" * (1 + (7 * k + k // 16) % 16) + b"\n+\n" + b"I" * (1 + (7 * k + k // 16) % 16) + b"\n" for k, h in enumerate(h1))
    return t0, t1


def header_offsets(t: bytes):
    at, out = 0, []
    for r in range(t.count(b"\n") // 4):
        out.append(at % 16)
        at = pm.end_of_record(t, r + 1)
    return out


def cases():
    A, B = b"@A", b"@B"
    one = lambda h: text([h])
    out = [
        ("empty_files", b"", b"", {}),
        ("one_record_each_mates", one(b"@a/1"), one(b"@a/2"), {}),
        ("one_record_each_not_mates", one(b"@a/1"), one(b"@b/2"), {}),
        ("file_2_empty", text([A, B]), b"", {}),
        ("file_1_empty", b"", text([A, B]), {}),
        ("no_shared_name", text([b"@x%d" % k for k in range(70)]), text([b"@y%d" % k for k in range(70)]), {}),
        ("three_lines_only", b"@A\nAC\n+\n", b"@A\nAC\n+\n", {}),
        ("no_final_newline", text([A, B])[:-1], text([A, B])[:-1], {}),
    ]
    for n in EDGE_SIZES:
        h0, h1 = mates_files(n)
        out.append(("all_mates_%d" % n, text(h0), text(h1, 5), {}))
        for pos in sorted({0, 63, 64, n - 1}):
            if pos >= n:
                continue
            out.append(("n%d_without_%d_of_file_1" % (n, pos), text(h0[:pos] + h0[pos + 1:]), text(h1, 5), {}))
            out.append(("n%d_without_%d_of_file_2" % (n, pos), text(h0), text(h1[:pos] + h1[pos + 1:], 5), {}))
    long_name = b"@" + b"n" * 300
    out += [
        ("keys_differ_in_the_last_byte", text([b"@name_a", b"@name_b", b"@name_c"]), text([b"@name_b", b"@name_d", b"@name_c"]), {}),
        ("comments_differ", text([b"@a 1:N:0:x", b"@b\tleft"]), text([b"@a 2:Y:9:other", b"@b right"]), {}),
        ("tab_against_space", text([b"@a\tx y"]), text([b"@a x\ty"]), {}),
        ("slash_1_2", text([b"@a/1"]), text([b"@a/2"]), {}),
        ("slash_1_against_bare", text([b"@x/1"]), text([b"@x"]), {}),
        ("bare_against_slash_2", text([b"@x"]), text([b"@x/2"]), {}),
        ("slash_1_against_slash_1", text([b"@x/1"]), text([b"@x/1"]), {}),
        ("slash_2_against_slash_1", text([b"@x/2"]), text([b"@x/1"]), {}),
        ("only_the_suffix", text([b"/1", A]), text([b"/2", A]), {}),
        ("empty_token", text([b" x", A]), text([b" x", A]), {}),
        ("empty_header_lines", text([b"", A, b""]), text([b"", b"", A]), {}),
        ("one_byte_headers", text([b"@", b"a", b"b"]), text([b"a", b"@", b"c"]), {}),
        ("long_names", text([long_name + b"x/1", long_name + b"y/1", A]), text([long_name + b"x/2", long_name + b"z/2", A]), {}),
        ("prefix_of_the_other", text([b"@abc", b"@abcd"]), text([b"@abcd", b"@abcde"]), {}),
        ("swapped_in_file_2", text([A, B, b"@C", b"@D"]), text([A, b"@C", B, b"@D"]), {}),
        ("file_2_reversed", text([A, B, b"@C"]), text([b"@C", B, A]), {}),
        ("twice_in_file_1_with_mate", text([b"@p", A, B, A]), text([b"@p", A, B]), {}),
        ("twice_in_file_1_without_mate", text([b"@p", A, B, A]), text([b"@p", B]), {}),
        ("three_times_in_file_1", text([b"@p", b"@q", A, A, B, A]), text([b"@p", A, B]), {}),
        ("twice_in_file_2_with_mate", text([b"@p", A, B]), text([b"@p", b"@q", A, B, A]), {}),
        ("twice_in_file_2_without_mate", text([b"@p", B]), text([b"@p", b"@q", A, B, A]), {}),
        ("three_times_in_file_2", text([b"@p", A]), text([A, b"@p", A, A]), {}),
        ("twice_in_both_files", text([b"@p", A, A]), text([B, b"@p", B]), {}),
        ("suffix_makes_the_key_twice", text([b"@x/1", b"@x"]), text([b"@x/2"]), {}),
        ("empty_keys_are_never_twice", text([b" a", b" b", b"/1", b"/1"]), text([b"/2", b"/2", b" a"]), {}),
    ]
    t0, t1 = aligned_headers()
    out.append(("headers_at_every_alignment", t0, t1, {}))
    h0, h1 = mates_files(150)
    out.append(("name_bits_2", text(h0[:40] + h0[55:]), text(h1[:100] + h1[101:], 3), dict(name_bits=2)))
    out.append(("name_bits_2_duplicate", text(h0[:70] + [h0[3]]), text(h1[:70], 3), dict(name_bits=2)))
    # the smallest legal table, and a probe chain from its last slot round to slot 0
    w = colliding_keys(2, 1, 2)
    out.append(("table_2_wraps", text([w[0]]), text([w[1]]), dict(table=2)))
    out.append(("table_2_one_pair", text([w[0]]), text([w[0]]), dict(table=2)))
    w = colliding_keys(4, 3, 3)
    out.append(("table_4_wraps", text([w[0], w[1]]), text([w[2], w[1]]), dict(table=4)))
    w = colliding_keys(8, 7, 4)
    out.append(("table_8_wraps_full", text(w), text(list(reversed(w))[:1] + [b"@v%d" % k for k in range(4)]), dict(table=8)))
    return out


def sequences():
    """(name, file 1, file 2, chunk ends of file 1, of file 2): inputs whose point lies in how the windows follow each other"""
    h0, h1 = mates_files(30)
    lonely = [b"@only1_%d" % k for k in range(6)]
    # a tail of waiting singles: the records of file 1 behind its last match in window 1 are decided one window later
    t0, t1 = text(h0[:10] + lonely + h0[10:]), text(h1, 2)
    cut0 = pm.end_of_record(t0, 14)  # (four of the lonely records are in the first window, behind the last match)
    cut1 = pm.end_of_record(t1, 10)
    out = [("waiting_singles_decided_a_window_later", t0, t1, [cut0, len(t0)], [cut1, len(t1)])]
    # one file at its end while the other goes on for several windows
    t0, t1 = text(h0[:5]), text(h1, 2)
    out.append(("file_1_ends_early", t0, t1, [len(t0)], pm.chunks_after_every_record(t1)[4::5] + [len(t1)]))
    out.append(("file_2_ends_early", t1, t0, pm.chunks_after_every_record(t1)[4::5] + [len(t1)], [len(t0)]))
    out.append(("file_2_empty_file_1_in_windows", t1, b"", pm.chunks_after_every_record(t1)[2::3] + [len(t1)], [0]))
    # chunks that end inside lines
    t0, t1 = text(h0[:3] + h0[4:]), text(h1[:20] + h1[22:], 2)
    out.append(("chunks_of_7_and_11_bytes", t0, t1, list(range(7, len(t0), 7)) + [len(t0)], list(range(11, len(t1), 11)) + [len(t1)]))
    return [(n, a, b, sorted(set(e0)), sorted(set(e1))) for n, a, b, e0, e1 in out]
