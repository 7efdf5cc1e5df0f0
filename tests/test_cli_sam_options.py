"""compseed_amd_cli --sam: the translation of the command line into cs_map_params_t, read back through --show-params (no GPU, no index),
against a table worked out from the reference's rules: getopt's parsing and the opt0 marks (main.cpp:233-330), update_a (main.cpp:130-143)
over mem_opt_init's values (comp_seed.cpp:26-58).  What the stages do not have is refused with status 1 and a message naming the option,
and the program without --sam is what it was."""
import os
import subprocess

import pytest

DEFAULTS = dict(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, pen_clip5=5, pen_clip3=5, w=100, zdrop=100, T=30, min_seed_len=19, split_factor=1.5, split_width=10, max_occ=500,
                max_mem_intv=20, max_chain_gap=10000, max_chain_extend=1 << 30, min_chain_weight=0, mask_level=0.5, drop_ratio=0.5, xa_drop_ratio=0.8, mask_level_redun=0.95,
                mapq_coef_len=50, max_xa_hits=5, max_xa_hits_alt=200, flags=0, threads=16, rg_id="", copy_comment=0, chunk_bases=10000000)
ALL, NO_MULTI, KEEP_SUPP_MAPQ, SOFTCLIP = 1, 2, 4, 8

TABLE = [
    ([], {}),
    (["-A", "2"], dict(a=2, b=8, T=60, o_del=12, e_del=2, o_ins=12, e_ins=2, zdrop=200, pen_clip5=10, pen_clip3=10)),   # everything not given is scaled
    (["-A", "2", "-B", "3", "-T", "20"], dict(a=2, b=3, T=20, o_del=12, e_del=2, o_ins=12, e_ins=2, zdrop=200, pen_clip5=10, pen_clip3=10)),   # the given ones stay
    (["-B", "3", "-A", "2", "-d", "7", "-L", "4"], dict(a=2, b=3, T=60, o_del=12, e_del=2, o_ins=12, e_ins=2, zdrop=7, pen_clip5=4, pen_clip3=4)),   # ... in any order
    (["-O", "5,7", "-E", "2,1"], dict(o_del=5, o_ins=7, e_del=2, e_ins=1)),
    (["-O", "5", "-E", "2", "-A", "3"], dict(a=3, b=12, T=90, o_del=5, o_ins=5, e_del=2, e_ins=2, zdrop=300, pen_clip5=15, pen_clip3=15)),
    (["-h", "3,100"], dict(max_xa_hits=3, max_xa_hits_alt=100)),
    (["-h", "7"], dict(max_xa_hits=7, max_xa_hits_alt=7)),
    (["-L", "3,3"], dict(pen_clip5=3, pen_clip3=3)),
    (["-a", "-M", "-q", "-Y"], dict(flags=ALL | NO_MULTI | KEEP_SUPP_MAPQ | SOFTCLIP)),
    (["-aY"], dict(flags=ALL | SOFTCLIP)),                                  # getopt: clustered switches
    (["-M"], dict(flags=NO_MULTI)),
    (["-q"], dict(flags=KEEP_SUPP_MAPQ)),
    (["-R", "@RG\\tID:g1\\tSM:s"], dict(rg_id="g1")),
    (["-C"], dict(copy_comment=1)),
    (["-k", "23", "-r", "2.5", "-y", "30", "-c", "77", "-s", "4"], dict(min_seed_len=23, split_factor=2.5, max_mem_intv=30, max_occ=77, split_width=4)),
    (["-k23", "-w5"], dict(min_seed_len=23, w=5)),                          # getopt: the value attached
    (["-w", "5", "-d", "60", "-D", "0.25", "-W", "9", "-N", "50", "-G", "5000", "-X", "0.75", "-T", "17", "-Q", "40"],
     dict(w=5, zdrop=60, drop_ratio=0.25, min_chain_weight=9, max_chain_extend=50, max_chain_gap=5000, mask_level=0.75, T=17, mapq_coef_len=40)),
    (["-t", "3"], dict(chunk_bases=30000000)),
    (["-t", "3", "-K", "1234"], dict(chunk_bases=1234)),
    (["-o", "x.sam", "-f", "y.sam", "-1", "-v", "3"], {}),                  # accepted and ignored
    (["-A", "1", "-B", "2", "-O", "6,9", "-E", "3,1", "-L", "2,2", "-w", "5", "-d", "60"], dict(b=2, o_del=6, o_ins=9, e_del=3, e_ins=1, pen_clip5=2, pen_clip3=2, w=5, zdrop=60)),
]

REFUSED = [(["-5"], "-5"), (["-V"], "-V"), (["-Q", "0"], "-Q"), (["-Q", "-3"], "-Q"), (["-L", "3,4"], "-L"), (["-p"], "-p"), (["-x", "pacbio"], "-x"), (["-H", "@CO\\tx"], "-H"),
           (["-I", "300"], "-I"), (["-j"], "-j"), (["-S"], "-S"), (["-P"], "-P"), (["-U", "9"], "-U"), (["-m", "3"], "-m"), (["-a5"], "-5"),
           (["--dump-seeds", "d.txt"], "--dump-seeds"), (["--no-sal"], "--no-sal"), (["-R", "ID:g1"], "-R"), (["-R", "@RG\\tSM:s"], "-R")]


@pytest.fixture(scope="module")
def cli():
    import compseed_amd as ca
    if not os.path.exists(ca.lib_path()):
        ca.build_library()
    return os.path.join(os.path.dirname(ca.lib_path()), "compseed_amd_cli")


def _show(cli, args):
    r = subprocess.run([cli, "--show-params"] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return dict(ln.split("=", 1) for ln in r.stdout.splitlines())


@pytest.mark.parametrize("args,changed", TABLE, ids=[" ".join(a) or "defaults" for a, _ in TABLE])
def test_show_params_against_the_table(cli, args, changed):
    got = _show(cli, args)
    want = dict(DEFAULTS, **changed)
    assert sorted(got) == sorted(want)
    for k, v in want.items():
        assert (got[k] == v) if isinstance(v, str) else (float(got[k]) == pytest.approx(v, rel=1e-6)) if isinstance(v, float) else (int(got[k]) == v), (k, got[k], v)


def test_show_params_needs_no_index_and_takes_the_whole_line(cli, tmp_path):
    got = _show(cli, ["--sam", str(tmp_path / "never.sam"), "-A", "2", str(tmp_path / "no_index"), str(tmp_path / "no_reads")])
    assert got["a"] == "2" and got["T"] == "60" and not os.path.exists(str(tmp_path / "never.sam"))


@pytest.mark.parametrize("args,option", REFUSED, ids=[" ".join(a) for a, _ in REFUSED])
def test_refused_options(cli, tmp_path, args, option):
    out = str(tmp_path / "o.sam")
    r = subprocess.run([cli, "--sam", out] + args + [str(tmp_path / "no_index"), str(tmp_path / "no_reads")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and option in r.stderr and r.stdout == "" and not os.path.exists(out)


def test_a_second_reads_file_is_refused(cli, tmp_path):
    r = subprocess.run([cli, "--sam", str(tmp_path / "o.sam"), "idx", "reads_1.fq", "reads_2.fq"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "reads_2.fq" in r.stderr and "paired-end" in r.stderr


def test_sam_without_its_two_arguments_and_unknown_options(cli, tmp_path):
    for args in (["--sam", str(tmp_path / "o.sam"), "idx"], ["--sam", str(tmp_path / "o.sam"), "-Z", "idx", "reads"], ["--sam", str(tmp_path / "o.sam"), "--nope", "idx", "reads"]):
        r = subprocess.run([cli] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--sam FILE" in r.stderr and not os.path.exists(str(tmp_path / "o.sam"))


USAGE = """Usage: compseed_amd_cli [options] <FM-index> <Reordered Reads>

Seeding options (same meaning as CompSeed / bwamem):
       -t INT        host threads of the reference; sets the default chunk size (-K) [1]
       -k INT        minimum seed length [19]
       -r FLOAT      look for internal seeds inside a seed longer than {-k} * FLOAT [1.5]
       -y INT        seed occurrence for the 3rd round seeding [20]
       -c INT        skip seeds with more than INT occurrences [500]
       -s INT        re-seed only SMEMs with at most INT occurrences [10]
       -K INT        process INT input bases in each batch [10000000 x -t]
GPU / output options:
       --gpus INT    number of MI355X to shard each batch over [all visible]
       --devices LIST   comma-separated device ordinal of every shard instead (an ordinal may repeat)
       --no-sal      stop after SMEM collection (no suffix-array lookup)
       --dump-seeds FILE   write `M read beg end x0 x1 x2` and `S read qbeg len rbeg` lines
Other CompSeed flags (-w -d -D -W -m -S -P -A -B -O -E -L -U -x -p -R -H -o -j -5 -q -v -T -h -a -C -V -Y -M -I)
belong to stages behind seeding; they are accepted and ignored.
"""


def test_without_sam_the_program_is_what_it_was(cli):
    for args in ([], ["only_an_index"], ["-w", "100", "-M", "only_an_index"]):
        r = subprocess.run([cli] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and r.stderr == USAGE and r.stdout == "", args
    r = subprocess.run([cli, "-G", "5", "idx", "reads"], capture_output=True, text=True, timeout=60)   # the seeding mode's own option set, as before
    assert r.returncode == 1 and r.stderr == "[E::main] unknown option -G\n" + USAGE
