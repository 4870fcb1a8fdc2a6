"""k_gzip's DEFLATE stream on the device: the checks of tests/gzip_stream.py (see tests/test_emu_gzip_stream.py) through the product library, and the
members byte for byte as recorded from the CPU emulation (tests/golden/gzip_members.json): a valid stream that differs is what a race would look like."""
import pytest

import gzip_stream as G
from dwgsim_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def session(golden_dir):
    s = G.Session(api.load(), golden_dir)
    yield s
    s.close()


@pytest.mark.parametrize("seed", [5, 6])
def test_fuzzed_fastq_like_text(session, seed):
    G.check_fuzz(session, seed, 60)


def test_chain_histograms_take_the_depth_limit(session):
    worst = G.check_chains(session)
    print(f"\nflattened codes: at most {worst:.3%} over the package-merge optimum (cap 1 %)")


def test_long_records_reach_distances_of_13_extra_bits(session):
    G.check_long_records(session)


def test_a_match_token_of_more_than_32_bits(session):
    assert G.check_wide_token(session) > 32


@pytest.mark.parametrize("name", [c[0] for c in G.SIMULATED])
def test_matches_earn_their_place_on_simulated_text(session, name):
    got = G.check_simulated(session, name)
    print("\n" + name + ": " + "; ".join(f"name-line bytes inside matches {c:.2f}, member / zlib level 1 {z:.3f}" for c, z in got))


def test_the_same_text_gives_the_same_bytes(session):
    G.check_determinism(session)


def test_members_are_the_recorded_ones(session):
    G.check_golden(session)
