"""cs_map_submit / cs_map_collect on the GPU: batches in flight on one mapper, through the binding (Mapper.submit / collect / in_flight) and
through `compseed_amd_cli --sam`, against the reference program's file for main100 (3,000 reads of 100 bases, tests/golden/samtext1) on the
g1 index.  The stream gives the file whatever the batch sizes; every order of four submits and four collects gives each batch the text
map_batch gave it; a collected result outlives what is submitted and finishes behind it; what a submit, a collect and map_batch refuse;
a batch that a stage refuses fails at its own collect and nothing around it; close() with batches in flight; the command line in chunks."""
import gzip
import itertools
import os
import subprocess
import time

import numpy as np
import pytest

import _cigar
import _data
import _sam

pytestmark = pytest.mark.gpu
EINVAL = -1


def _raw():
    return gzip.open(os.path.join(_sam.DIR, "main100.default.sam.gz"), "rb").read()


def _mapper():
    import compseed_amd as ca
    return ca.Mapper(_data.PREFIX, 0, None, ca.MapParams())


def _batch(r0, r1):
    """reads [r0, r1) of main100 as submit's arguments, id_base carried"""
    i = _sam.inputs("main100")
    off = i["off"].astype(np.int64)
    nb, no = i["names"][0], i["names"][1].astype(np.int64)
    return dict(bases=i["bases"][off[r0]:off[r1]], read_offsets=(off[r0:r1 + 1] - off[r0]).astype(np.uint64),
                names=(nb[no[r0]:no[r1]], (no[r0:r1 + 1] - no[r0]).astype(np.uint64)), id_base=r0)


def _ranges(sizes):
    r0, out = 0, []
    for k in sizes:
        out.append((r0, r0 + k)); r0 += k
    return out


def test_stream_equals_the_file():
    """main100 as batches of 1, 63, 64, 65, 1000, none, 1700 and the last 107 reads, three kept in flight: header + the texts in order is
    the reference program's file, and the counters are the manifest's"""
    import compseed_amd as ca
    e = _sam.MANIFEST["files"]["main100.default.sam.gz"]
    n = _sam.inputs("main100")["off"].size - 1
    sizes = [1, 63, 64, 65, 1000, 0, 1700]
    sizes.append(n - sum(sizes))
    assert sizes[-1] == 107 and ca.MAP_MAX_IN_FLIGHT == 3
    ranges, parts, peak = _ranges(sizes), [], 0
    m = _mapper()
    try:
        header = m.header()
        nxt = 0
        while len(parts) < len(ranges):
            while nxt < len(ranges) and m.in_flight()[0] < ca.MAP_MAX_IN_FLIGHT:
                m.submit(**_batch(*ranges[nxt])); nxt += 1
            sub, fin = m.in_flight()
            assert 0 <= fin <= sub <= ca.MAP_MAX_IN_FLIGHT
            peak = max(peak, sub)
            text_off, text = m.collect()
            k = sizes[len(parts)]
            assert text_off.size == k + 1 and int(text_off[-1]) == len(text) and (k or (text == b"" and text_off.tolist() == [0]))
            parts.append(text)
        assert m.in_flight() == (0, 0)
        st = m.stats()
    finally:
        m.close()
    assert peak == 3
    assert header + b"".join(parts) == _raw()
    assert (st["reads"], st["lines"] + st["unmapped"], st["unmapped"], st["bytes"], st["batches"]) == (n, e["lines"], e["unmapped"], e["raw_bytes"] - len(header), len(sizes) - 1)
    assert st["bases"] == int(_sam.inputs("main100")["off"][-1]) and st["regions"] >= st["lines"] and all(v > 0 for v in st["stage_ms"].values())


def _schedules(n, cap):
    """every order of n submits ('s') and n collects ('c') with at most `cap` in flight and no collect on an empty stream"""
    out = []
    for seq in itertools.product("sc", repeat=2 * n):
        fl, ok = 0, seq.count("s") == n
        for x in seq:
            fl += 1 if x == "s" else -1
            ok = ok and 0 <= fl <= cap
        if ok:
            out.append("".join(seq))
    return out


def test_every_schedule():
    """batches of 40, 0, 64 and 200 reads in every order of four submits and four collects: each collect hands out, in submission order,
    the text map_batch gave that batch on the same mapper beforehand"""
    import compseed_amd as ca
    ranges = _ranges([40, 0, 64, 200])
    scheds = _schedules(4, ca.MAP_MAX_IN_FLIGHT)
    assert len(scheds) == 13 and "sssccscc" in scheds and "sssscccc" not in scheds   # the Catalan number 14 less the one schedule with four in flight
    m = _mapper()
    try:
        want = [m.map_batch(**_batch(*r)) for r in ranges]
        assert want[1][1] == b"" and all(len(w[1]) for k, w in enumerate(want) if k != 1)
        for sched in scheds:
            s = c = 0
            for x in sched:
                if x == "s":
                    m.submit(**_batch(*ranges[s])); s += 1
                else:
                    text_off, text = m.collect()
                    assert text == want[c][1] and text_off.tolist() == want[c][0].tolist(), (sched, c)
                    c += 1
                assert m.in_flight()[0] == s - c
    finally:
        m.close()


def test_a_collected_result_outlives_what_finishes_behind_it():
    import compseed_amd as ca
    ranges = _ranges([300, 700, 500])
    m = _mapper()
    try:
        want = [m.map_batch(**_batch(*r))[1] for r in ranges]
        m.submit(**_batch(*ranges[0]))
        text_off, view = m.collect(copy=False)                             # the mapper's own arrays, not a copy
        assert isinstance(view, np.ndarray) and not view.flags["OWNDATA"] and view.tobytes() == want[0] and int(text_off[-1]) == view.size
        m.submit(**_batch(*ranges[1])); m.submit(**_batch(*ranges[2]))
        deadline = time.monotonic() + 60
        while m.in_flight() != (2, 2):
            assert time.monotonic() < deadline, m.in_flight()
            time.sleep(0.001)
        assert view.tobytes() == want[0]                                    # two batches went through every stage meanwhile
        del view, text_off                                                  # the next collect ends the claim
        assert m.collect()[1] == want[1] and m.collect()[1] == want[2]
    finally:
        m.close()


def _raises(fn, code=EINVAL):
    import compseed_amd as ca
    with pytest.raises(ca.CSError) as ei:
        fn()
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    return str(ei.value)


def test_errors():
    import compseed_amd as ca
    ranges = _ranges([50, 60, 70])
    m = _mapper()
    try:
        want = [m.map_batch(**_batch(*r))[1] for r in ranges]
        _raises(m.collect)                                                  # nothing in flight
        m.submit(**_batch(*ranges[0]))
        bad = _batch(*ranges[1]); bad["read_offsets"] = bad["read_offsets"].copy(); bad["read_offsets"][7] = bad["read_offsets"][6] - 1
        assert "read_offsets decreases" in _raises(lambda: m.submit(**bad)) and m.in_flight()[0] == 1   # refused at submit; the stream as it was
        assert "in flight" in _raises(lambda: m.map_batch(**_batch(*ranges[1]))) and m.in_flight()[0] == 1
        # a name_off that dips in the middle and ends where it should: cs_map_submit's checks look at read_offsets only, no stage before the
        # SAM stage reads the names, and there the checking kernel refuses offsets that are not a CSR array before any kernel follows one
        dip = _batch(*ranges[1]); nb, no = dip["names"]; no = no.copy(); no[30] = no[29] - 1; dip["names"] = (nb, no)
        assert no[-1] == nb.size and no[30] < no[29]
        m.submit(**dip)
        m.submit(**_batch(*ranges[2]))
        assert "CS_MAP_MAX_IN_FLIGHT" in _raises(lambda: m.submit(**_batch(*ranges[0]))) and m.in_flight()[0] == 3   # a fourth
        _, view = m.collect(copy=False)
        assert view.tobytes() == want[0]                                    # the batch before it
        msg = _raises(m.collect)                                            # fails at its own collect, the stage named
        assert "cs_map_collect: SAM text: cs_regions_sam" in msg and m.in_flight()[0] == 1
        assert view.tobytes() == want[0]                                    # ... which did not shorten the life of the result before
        del view
        assert m.collect()[1] == want[2]                                    # the batch behind it
        _raises(m.collect)
        st = m.stats()
        assert st["batches"] == 3 + 2 and st["reads"] == 180 + 50 + 70     # the refused batch adds nothing
        m.submit(**_batch(*ranges[1]))                                      # the mapper is usable: streamed and blocking
        assert m.collect()[1] == want[1] and m.map_batch(**_batch(*ranges[0]))[1] == want[0]
    finally:
        m.close()


def test_close_with_batches_uncollected():
    m = _mapper()
    m.submit(**_batch(0, 400)); m.submit(**_batch(400, 900))
    assert m.in_flight()[0] == 2
    m.close()                                                               # waits for them and returns
    assert not m.h


@pytest.mark.parametrize("args", [["-K", "30000"], ["-K", "30000", "--devices", "0,0"]], ids=["-K 30000", "-K 30000 --devices 0,0"])
def test_command_line_in_ten_chunks(tmp_path, args):
    import compseed_amd as ca
    cli = os.path.join(os.path.dirname(ca.lib_path()), "compseed_amd_cli")
    reads = os.path.join(_cigar.DDP1["main100"], "main100.txt")
    rd = ca.Reader(reads, 30000); chunks = 0
    try:
        while rd.next_chunk() is not None:
            chunks += 1
    finally:
        rd.close()
    assert chunks == 10
    out = str(tmp_path / "out.sam")
    r = subprocess.run([cli, "--sam", out] + args + [_data.PREFIX, reads], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(out, "rb").read() == _raw()
    assert "SAM:         3000 reads, %d lines" % _sam.MANIFEST["files"]["main100.default.sam.gz"]["lines"] in r.stderr
