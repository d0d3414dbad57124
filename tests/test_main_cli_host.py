"""main.py's command line, which it reads off the table of the record front end (frontend.STAGES): per stage, what its
options make of Settings and what the run prints - the checks that stood with each stage's host tests; every argument list
the command line refuses, as a usage error that names the stage's option or setting; the 56 chains of tests/chain_cases.py
spelled as arguments, against the accept / refuse table of tests/test_chain_host.py; and the options against the table.
postProcessing is stubbed: nothing here needs a GPU.  Run with -m "not gpu"."""
import importlib
import re

import pytest

import chain_cases as cases
from conftest import pkg
from test_chain_host import verdicts


@pytest.fixture(scope="module")
def built():
    importlib.import_module("__graft_entry__").build()
    return pkg()


def stage(name):
    return dict((s.name, s) for s in pkg("frontend").STAGES)[name]


# ---- per stage: what its options make of the settings postProcessing receives ------------------------------------------------
# look: what the stub keeps of the settings; clear: whether it forgets the run before; steps: (arguments, what `seen` must
# be - a dict: all of it; a function: what it says of `seen` - and what stdout must hold); doc: what main.__doc__ must name
OPTIONS = {
    "unpack": dict(
        look=lambda s: dict(bits=s.packedBits, enc=s.packedEncoding, lsb=s.packedLsbFirst, frame=s.packedFrame,
                            first=s.packedFirst, peak=s.packedPeak, iq=s.iqRecord, dataType=s.dataType,
                            skip=s.skipNumberOfBytes),
        clear=True,
        steps=[
            (["x.bin", "--no-probe", "--packed", "2", "--iq", "--fs", "4096000", "--IF", "0"],
             dict(bits=2, enc="sign-magnitude", lsb=False, frame=1, first=0, peak=48, iq=True, dataType="int8", skip=0), ()),
            (["x.bin", "--no-probe", "--packed", "4", "--packed-encoding", "twos-complement", "--packed-lsb-first",
              "--packed-frame", "4:2", "--packed-peak", "63", "--iq", "--skip", "2000"],
             dict(bits=4, enc="twos-complement", lsb=True, frame=4, first=2, peak=63, iq=True, dataType="int8", skip=2000), ()),
            (["x.bin", "--no-probe", "--packed", "1", "--packed-frame", "8"],
             lambda seen: (seen["bits"], seen["frame"], seen["first"], seen["iq"]) == (1, 8, 0, False), ()),
            (["x.bin", "--no-probe"], lambda seen: seen["bits"] == 0, ()),
        ],
        doc=("--packed", "--packed-frame")),
    "condition": dict(
        look=lambda s: dict(on=s.frontEndConditioning, c=s.condBlankFactor, iq=s.iqRecord, dataType=s.dataType),
        clear=False,
        steps=[
            (["x.bin", "--no-probe", "--iq", "--dtype", "int16", "--condition"],
             dict(on=True, c=4.0, iq=True, dataType="int16"), ()),
            (["x.bin", "--no-probe", "--dtype", "int16", "--condition=3.5"],
             dict(on=True, c=3.5, iq=False, dataType="int16"), ()),
            (["x.bin", "--no-probe", "--condition=0"], dict(on=True, c=0.0, iq=False, dataType="int8"), ()),
            (["x.bin", "--no-probe"], lambda seen: seen["on"] is False, ()),
        ],
        doc=("--condition",)),
    "requantise": dict(
        look=lambda s: dict(iqRecord=s.iqRecord, iqRequantize=s.iqRequantize, iqTargetRms=s.iqTargetRms,
                            dataType=s.dataType, skip=s.skipNumberOfBytes),
        clear=False,
        steps=[
            (["x.bin", "--no-probe", "--iq", "--dtype", "int16", "--iq-requantize", "--skip", "4000"],
             dict(iqRecord=True, iqRequantize=True, iqTargetRms=12.0, dataType="int16", skip=4000), ()),
            (["x.bin", "--no-probe", "--iq=qi", "--dtype", "float32", "--iq-requantize=20.5"],
             dict(iqRecord=True, iqRequantize=True, iqTargetRms=20.5, dataType="float32", skip=0), ()),
            (["x.bin", "--no-probe", "--iq"], lambda seen: seen["iqRequantize"] is False and seen["dataType"] == "int8", ()),
        ],
        doc=("--iq-requantize",)),
    "decimate": dict(
        look=lambda s: dict(D=s.decimation, taps=s.decimTaps, bw=s.decimBandwidth, gain=s.decimGain, iq=s.iqRecord,
                            fs=s.samplingFreq, IF=s.IF, skip=s.skipNumberOfBytes),
        clear=True,
        steps=[
            (["x.bin", "--no-probe", "--iq", "--fs", "16368000", "--IF", "3200000", "--decimate", "4"],
             dict(D=4, taps=127, bw=2.046e6, gain=0.0, iq=True, fs=16368000.0, IF=3200000.0, skip=0),
             ("8.184000 Msps", "1.154000 MHz")),
            (["x.bin", "--no-probe", "--decimate", "5:63", "--decimate-bandwidth", "2.4e6", "--skip", "500"],
             dict(D=5, taps=63, bw=2.4e6, gain=0.0, iq=False, fs=38192000.0, IF=9548000.0, skip=500), ()),
            (["x.bin", "--no-probe"], lambda seen: seen["D"] == 0, ()),
        ],
        doc=("--decimate", "--decimate-bandwidth")),
    "resample": dict(
        look=lambda s: dict(L=s.resampleUp, M=s.resampleDown, taps=s.resampTaps, cutoff=s.resampCutoff, gain=s.resampGain,
                            fs=s.samplingFreq, IF=s.IF, skip=s.skipNumberOfBytes),
        clear=True,
        steps=[
            (["x.bin", "--no-probe", "--fs", "4096000", "--IF", "1000000", "--resample", "10"],
             dict(L=10, M=1, taps=0, cutoff=0.0, gain=1.0, fs=4096000.0, IF=1000000.0, skip=0),
             ("40.960000 Msps", "1.000000 MHz")),
            (["x.bin", "--no-probe", "--fs", "16368000", "--IF", "4092000", "--resample", "7/3:127", "--resample-cutoff", "7e6",
              "--skip", "300"],
             dict(L=7, M=3, taps=127, cutoff=7e6, gain=1.0, fs=16368000.0, IF=4092000.0, skip=300), ("38.192000 Msps",)),
            (["x.bin", "--no-probe", "--fs", "4096000", "--IF", "1000000", "--resample", "10:121"],
             lambda seen: (seen["L"], seen["M"], seen["taps"]) == (10, 1, 121), ()),
            (["x.bin", "--no-probe"], lambda seen: seen["L"] == 0, ()),
        ],
        doc=("--resample", "--resample-cutoff")),
}


@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_stage_options(built, monkeypatch, capsys, name):
    main = pkg("main")
    case = OPTIONS[name]
    seen = {}

    def fake_post(self, fileNameStr=None):
        if case["clear"]:
            seen.clear()
        seen.update(case["look"](self))
        return None, None, None

    monkeypatch.setattr(built.Settings, "postProcessing", fake_post)
    for argv, want, printed in case["steps"]:
        assert main.main(argv) == 0
        if isinstance(want, dict):
            assert seen == want, argv
        else:
            assert want(seen), (argv, seen)
        out = capsys.readouterr().out
        for text in printed:
            assert text in out, (argv, text)
    for option in case["doc"]:
        assert option in main.__doc__


def test_decimate_in_front_of_the_converter_shows_the_converter_s_line(built, monkeypatch, capsys):
    """The banner is the line of the last stage that is on and has one, at the prepared rate and IF."""
    monkeypatch.setattr(built.Settings, "postProcessing", lambda self, fileNameStr=None: (None, None, None))
    main = pkg("main")
    assert main.main(["x.bin", "--no-probe", "--iq", "--fs", "16368000", "--IF", "3200000", "--decimate", "4"]) == 0
    assert capsys.readouterr().out.splitlines()[3] == \
        "I/Q record at 16.368000 Msps, carrier at +3.200000 MHz: read as a real record at 8.184000 Msps, IF 1.154000 MHz"
    assert main.main(["x.bin", "--no-probe", "--decimate", "5"]) == 0
    assert capsys.readouterr().out.splitlines()[3] == \
        "Decimated by 5: read as a real record at 7.638400 Msps, IF 1.909600 MHz"


# ---- the refusals ------------------------------------------------------------------------------------------------------------
# (the stage whose option or Settings attribute the message names, the arguments): every argument list the stages' host tests
# held to be refused, then those the package refuses and main.main once let through or answered with a traceback
REFUSED = [
    ("unpack", ["x.bin", "--packed", "3"]), ("unpack", ["x.bin", "--packed-peak", "48"]),
    ("unpack", ["x.bin", "--packed-lsb-first"]), ("unpack", ["x.bin", "--packed", "2", "--packed-frame", "3"]),
    ("unpack", ["x.bin", "--packed", "2", "--packed-frame", "4:4"]),
    ("unpack", ["x.bin", "--packed", "2", "--iq", "--packed-frame", "4:3"]),
    ("unpack", ["x.bin", "--packed", "2", "--packed-frame", "x"]), ("unpack", ["x.bin", "--packed", "2", "--packed-peak", "2"]),
    ("unpack", ["x.bin", "--packed", "2", "--packed-peak", "128"]),
    ("unpack", ["x.bin", "--packed", "2", "--packed-encoding", "gray"]), ("unpack", ["x.bin", "--packed", "2", "--condition"]),
    ("unpack", ["x.bin", "--packed", "2", "--iq", "--iq-requantize"]), ("unpack", ["x.bin", "--packed", "2", "--dtype", "int16"]),
    ("condition", ["x.bin", "--condition=0.5"]), ("condition", ["x.bin", "--condition=17"]),
    ("condition", ["x.bin", "--iq", "--iq-requantize", "--condition"]),
    ("requantise", ["x.bin", "--iq-requantize"]), ("requantise", ["x.bin", "--iq", "--iq-requantize=0"]),
    ("requantise", ["x.bin", "--iq", "--iq-requantize=128"]),
    ("decimate", ["x.bin", "--decimate", "1"]), ("decimate", ["x.bin", "--decimate", "17"]),
    ("decimate", ["x.bin", "--decimate", "5:64"]), ("decimate", ["x.bin", "--decimate", "5:513"]),
    ("decimate", ["x.bin", "--decimate", "x"]), ("decimate", ["x.bin", "--decimate", "5:63:2"]),
    ("decimate", ["x.bin", "--decimate-bandwidth", "2e6"]),
    ("decimate", ["x.bin", "--decimate", "5", "--decimate-bandwidth", "0"]),
    ("decimate", ["x.bin", "--decimate", "5", "--correlator-bank", "0:1:0.5"]),
    ("resample", ["x.bin", "--resample", "1"]), ("resample", ["x.bin", "--resample", "17"]),
    ("resample", ["x.bin", "--resample", "4/2"]), ("resample", ["x.bin", "--resample", "7/4"]),
    ("resample", ["x.bin", "--resample", "2/3"]), ("resample", ["x.bin", "--resample", "10:240"]),
    ("resample", ["x.bin", "--resample", "10:1025"]), ("resample", ["x.bin", "--resample", "x"]),
    ("resample", ["x.bin", "--resample", "10/1:121:2"]), ("resample", ["x.bin", "--resample", "10/"]),
    ("resample", ["x.bin", "--resample-cutoff", "2e6"]), ("resample", ["x.bin", "--resample", "10", "--resample-cutoff", "0"]),
    ("resample", ["x.bin", "--resample", "10", "--correlator-bank", "0:1:0.5"]),
    # refused by the package all along, by main.main only now: a traceback out of the banner, or a run that failed later
    ("decimate", ["x.bin", "--no-probe", "--decimate", "2"]),                  # the default record's IF sits on a zone edge
    ("decimate", ["x.bin", "--no-probe", "--decimate", "3", "--skip", "1"]),
    ("decimate", ["x.bin", "--no-probe", "--dtype", "int16", "--decimate", "3"]),
    ("resample", ["x.bin", "--no-probe", "--resample", "5/3", "--fs", "4096000", "--IF", "3000000"]),
    ("convert", ["x.bin", "--no-probe", "--iq", "--skip", "1"]),
    ("condition", ["x.bin", "--no-probe", "--dtype", "float32", "--condition"]),
    ("unpack", ["x.bin", "--no-probe", "--packed", "2", "--condition"]),
    # what the option's own syntax must refuse, because to Settings a 0 means "off" or "the default length"
    ("decimate", ["x.bin", "--decimate", "0"]), ("resample", ["x.bin", "--resample", "0"]),
    ("resample", ["x.bin", "--resample", "10:0"]),
    # the third stage whose record --correlator-bank cannot replay from the file
    ("convert", ["x.bin", "--iq", "--correlator-bank", "0:1:0.5"]),
]


def named(text, word):
    return re.search(r"(?<![\w-])%s(?![\w-])" % re.escape(word), text) is not None


@pytest.mark.parametrize("name,argv", REFUSED, ids=[" ".join(argv[1:]) for _, argv in REFUSED])
def test_refused_as_a_usage_error(built, monkeypatch, capsys, name, argv):
    """SystemExit(2) before anything is probed or opened, and the message - what follows argparse's usage lines - names an
    option of the stage or one of its settings."""
    def never(self, *args, **kw):
        raise AssertionError("the run went on")

    for method in ("postProcessing", "probeData", "_prepared_record"):
        monkeypatch.setattr(built.Settings, method, never)
    with pytest.raises(SystemExit) as e:
        pkg("main").main(argv)
    assert e.value.code == 2
    captured = capsys.readouterr()
    message = captured.err.split(": error: ", 1)[1]
    words = [flag for flag, _ in stage(name).options] + ["Settings." + k for k, _ in stage(name).defaults]
    assert any(named(message, w) for w in words), (name, message)
    assert "Welcome" not in captured.out and "Traceback" not in captured.err


# ---- the chains of tests/chain_cases.py as argument lists ---------------------------------------------------------------------

def chain_args(c):
    args = ["x.bin", "--no-probe", "--fs", repr(c.fs), "--IF", repr(c.f0), "--dtype", c.dtype]
    args += {"none": [], "packed": ["--packed", str(c.bits)], "cond": ["--condition"], "requant": ["--iq-requantize"]}[c.first]
    if c.iq:
        args += ["--iq"]
    if c.D:
        args += ["--decimate", str(c.D)]
    if c.resamp:
        args += ["--resample", "%d/%d" % c.resamp]
    return args


@pytest.mark.parametrize("chain,verdict", verdicts(), ids=[c.name for c, _ in verdicts()])
def test_a_chain_as_arguments(built, monkeypatch, capsys, chain, verdict):
    """An accepted chain reaches postProcessing with the settings chain.settings() writes by hand; requantise without iq -
    refused by _walk(), or switching nothing on - is a usage error: the early refusals take nothing away that runs."""
    got = {}
    monkeypatch.setattr(built.Settings, "postProcessing", lambda self, fileNameStr=None: got.update(vars(self)) or (None,) * 3)
    main = pkg("main")
    if verdict != "A":
        assert chain.first == "requant" and not chain.iq
        with pytest.raises(SystemExit) as e:
            main.main(chain_args(chain))
        assert e.value.code == 2 and not got
        assert named(capsys.readouterr().err.split(": error: ", 1)[1], "--iq-requantize")
        return
    assert main.main(chain_args(chain)) == 0
    want = chain.settings(built)
    for k in [k for k, _ in pkg("frontend").DEFAULTS] + ["samplingFreq", "IF", "dataType"]:
        assert got[k] == getattr(want, k), (chain.name, k, got[k], getattr(want, k))


# ---- the options against the table --------------------------------------------------------------------------------------------

def test_every_option_of_the_table_is_offered_and_described(built, capsys):
    main = pkg("main")
    with pytest.raises(SystemExit) as e:
        main.main(["--help"])
    assert e.value.code == 0
    offered = capsys.readouterr().out
    owners = {}
    for s in pkg("frontend").STAGES:
        assert s.options and s.usage.startswith(s.options[0][0])                # the option that switches it on comes first
        for flag, keywords in s.options:
            assert "help" in keywords and named(offered, flag) and named(main.__doc__, flag), flag
            assert flag not in owners, (flag, owners[flag], s.name)             # no option belongs to two entries
            owners[flag] = s.name
    # in the table's order, behind the options that are no stage's
    places = [offered.index("\n  %s " % flag) for flag in owners]
    assert places == sorted(places) and offered.index("\n  --dtype ") < places[0]
