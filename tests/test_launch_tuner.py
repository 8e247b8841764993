"""The launcher's timed A/B tuners (tile shape: two rounds, light split: one) without a GPU: rm_internal.h's tune_schedule and
tune_decide, compiled with plain g++ into a small driver that answers one query per input line."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r'''
#include <cstdio>
#include "rm_internal.h"
// "s rounds frame"            -> "candidate slot"
// "d rounds allRead t0 t1 ..." -> "candidate"
int main() {
  char op;
  while (std::scanf(" %c", &op) == 1) {
    int rounds = 0;
    if (std::scanf("%d", &rounds) != 1) return 2;
    if (op == 's') {
      int frame = 0;
      if (std::scanf("%d", &frame) != 1) return 2;
      const rm::TuneStep t = rm::tune_schedule(frame, rounds);
      std::printf("%d %d\n", t.candidate, t.slot);
    } else {
      int allRead = 0;
      float ms[4] = {};
      if (std::scanf("%d", &allRead) != 1) return 2;
      for (int k = 0; k < 2 * rounds; k++) if (std::scanf("%f", &ms[k]) != 1) return 2;
      std::printf("%d\n", rm::tune_decide(ms, rounds, allRead != 0));
    }
  }
  return 0;
}
'''


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    d = tmp_path_factory.mktemp("tuner")
    src, exe = d / "tuner.cpp", d / "tuner"
    src.write_text(DRIVER)
    cmd = ["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "raymarcher_amd", "csrc"), str(src), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]

    def run(lines):
        r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (r.returncode, r.stderr[-500:])
        return r.stdout.split("\n")[:len(lines)]
    return run


def schedule(driver, rounds, frames):
    return [tuple(map(int, line.split())) for line in driver([f"s {rounds} {f}" for f in frames])]


def test_tile_shape_schedule_two_rounds(driver):
    # frames 0-1, 4-5: candidate 0 (8×8); 2-3, 6-7: candidate 1 (4×16); the odd frames timed in slot 2·round + candidate
    expect = [(0, -1), (0, 0), (1, -1), (1, 1), (0, -1), (0, 2), (1, -1), (1, 3)]
    assert schedule(driver, 2, range(8)) == expect
    # from frame 8 until the timings are in: candidate 0, untimed
    assert schedule(driver, 2, range(8, 40)) == [(0, -1)] * 32


def test_light_split_schedule_one_round(driver):
    # frames 0-1 plain, 2-3 split, frames 1 and 3 timed; then plain while the timings are outstanding
    assert schedule(driver, 1, range(4)) == [(0, -1), (0, 0), (1, -1), (1, 1)]
    assert schedule(driver, 1, range(4, 20)) == [(0, -1)] * 16


def decide(driver, rounds, all_read, times):
    return int(driver([f"d {rounds} {1 if all_read else 0} " + " ".join(repr(float(t)) for t in times)])[0])


def test_candidate_one_must_win_by_three_percent(driver):
    assert decide(driver, 1, True, [1.0, 0.96]) == 1
    assert decide(driver, 1, True, [1.0, 0.975]) == 0
    assert decide(driver, 1, True, [1.0, 1.0]) == 0     # a tie keeps candidate 0
    assert decide(driver, 1, True, [1.0, 1.5]) == 0
    assert decide(driver, 2, True, [2.0, 1.9, 2.0, 1.9]) == 1
    assert decide(driver, 2, True, [2.0, 1.96, 2.0, 1.96]) == 0


def test_each_candidate_is_judged_by_its_best_round(driver):
    # slots: [c0 round 0, c1 round 0, c0 round 1, c1 round 1]
    assert decide(driver, 2, True, [5.0, 1.9, 2.0, 5.0]) == 1   # minima 2.0 / 1.9: candidate 1's best wins by 5 %
    assert decide(driver, 2, True, [1.0, 1.9, 5.0, 5.0]) == 0   # candidate 0's best round (1.0) decides, not its worse one
    assert decide(driver, 2, True, [5.0, 5.0, 2.0, 1.9]) == 1
    assert decide(driver, 2, True, [2.0, 5.0, 5.0, 1.98]) == 0  # 1.98 is within 3 % of 2.0


def test_an_unreadable_time_keeps_candidate_zero(driver):
    assert decide(driver, 1, False, [1.0, 0.5]) == 0
    assert decide(driver, 2, False, [1.0, 0.5, 1.0, 0.5]) == 0
