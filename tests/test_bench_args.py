"""bench.py's options (CPU): a plain run is the headline alone, `--full` keeps every leg as its switches say, and the options
that only shape a --full leg are refused without it instead of being dropped in silence."""
import pytest

import bench

LEGS = ("no_cpu_baseline", "no_default_aligner_leg", "no_upstream_check", "no_shard_leg", "no_stream_leg", "no_polish_leg")


def test_plain_run_switches_every_leg_off():
    a = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "2", "--dump-outputs", "d"])
    assert a.full is False and all(getattr(a, k) for k in LEGS), a
    assert a.bam_leg == "none" and a.loci == 0 and not a.files_leg
    assert (a.steps, a.warmup, a.dump_outputs, a.config) == (3, 2, "d", "c2")


def test_full_run_keeps_the_defaults_and_the_switches():
    a = bench.parse(["--full"])
    assert a.full is True and not any(getattr(a, k) for k in LEGS), a
    assert a.bam_leg == "device" and a.loci == -1 and (a.steps, a.warmup) == (8, 1)
    a = bench.parse(["--full", "--no-cpu-baseline", "--loci", "30", "--bam-leg", "host", "--files-leg", "--poa-parity", "5"])
    assert a.no_cpu_baseline and not a.no_default_aligner_leg and a.loci == 30 and a.bam_leg == "host" and a.files_leg and a.poa_parity == 5


@pytest.mark.parametrize("opt", [["--files-leg"], ["--flank-parity"], ["--poa-parity", "10"], ["--bam-sha"], ["--force-exchange"]])
def test_options_of_full_legs_need_full(opt, capsys):
    with pytest.raises(SystemExit) as e:
        bench.parse(opt)
    assert e.value.code == 2 and "--full" in capsys.readouterr().err
    assert bench.parse(opt + ["--full"]).full is True
