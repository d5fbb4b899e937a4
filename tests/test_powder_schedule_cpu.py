"""The medium/hard powderworld launch schedule (ogbench_amd/csrc/powder_schedule.h).

Results never depend on the schedule (tests/test_powder_full_gpu.py pins that),
so a wrong order_mode or a needless pwf_order_kernel would pass every GPU
test.  Here pwf_plan_step is enumerated on the CPU through a stand-alone driver
(tests/powder_schedule_main.cpp) and compared with a restatement of the rule
written from what the kernels need, in terms of one in-phase env's stage and
elapsed steps rather than the header's modular arithmetic.
"""
import itertools
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, '..', 'ogbench_amd', 'csrc')


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no system C++ compiler'
    d = tmp_path_factory.mktemp('pwsched')
    exe = str(d / 'powder_schedule_main')
    base = [cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-I', CSRC,
            os.path.join(HERE, 'powder_schedule_main.cpp'), '-o', exe]
    san = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    # with the sanitizers where this machine can link them (stand-alone program: nothing preloaded)
    if subprocess.run(base + san, capture_output=True).returncode != 0:
        subprocess.run(base, check=True)

    def run(cases):
        text = ''.join(' '.join(map(str, (c['phase'], c['max_steps'], c['auto_reset'], c['light'], c['fits'],
                                          len(c['ks']), *c['ks']))) + '\n' for c in cases)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
        blocks = [b.strip().split('\n') for b in out.split('case\n')[1:]]
        assert len(blocks) == len(cases)
        return blocks

    return run


class Model:
    """What the host may conclude about a batch whose envs were all reset
    `phase` steps ago (phase < 0: nothing is known)."""

    def __init__(self, phase, max_steps, auto_reset, light, fits):
        self.T, self.auto, self.light_enabled, self.fits = max_steps, auto_reset, light, fits
        self.phase = phase
        self.pending = None  # key of the order the last light launch pre-sorted: None, 'cost' or 'task'
        self.el, self.stage = 0, 0  # an in-phase env: elapsed steps and stage of the 3-step action machine
        for _ in range(max(phase, 0)):
            self.el, self.stage = self.after(self.el, self.stage)

    def needs(self, el, stage):
        """(forward, auto-reset) of an env's next step.  max_steps <= 0 is
        rejected by create; the plan treats it as no episode limit."""
        return stage == 2, bool(self.auto and self.T > 0 and el + 1 >= self.T)

    def after(self, el, stage):
        return (0, 0) if self.needs(el, stage)[1] else (el + 1, (stage + 1) % 3)

    def step(self, k):
        known = self.phase >= 0
        fwd = rst = False
        if known and k == 1:
            fwd, rst = self.needs(self.el, self.stage)
        full = fwd or rst  # every in-phase env needs the full kernel (a fused call: not known)
        # the light kernel steps one step's render-only envs: worth a launch unless no in-phase env is one
        light = bool(self.light_enabled and k == 1 and not full)
        mode = 0
        if light and known and self.fits:
            # the step before an in-phase full step sorts for it
            nf, nr = self.needs(*self.after(self.el, self.stage))
            mode = 2 if nr else 1 if nf else 0
        sparse = light and known  # in phase, the light kernel leaves (nearly) nothing
        use_order = known and k == 1 and full and bool(self.fits)
        by_task = use_order and rst
        run_order = use_order and self.pending != ('task' if by_task else 'cost')
        self.pending = {0: None, 1: 'cost', 2: 'task'}[mode]
        if known:
            for _ in range(k):
                self.el, self.stage = self.after(self.el, self.stage)
            self.phase += k
        plan = [light, mode, sparse, light and not sparse, use_order, run_order, by_task]
        return [int(x) for x in plan], self.phase, int(self.pending is not None), int(self.pending == 'task')


def _check(driver, cases):
    for c, lines in zip(cases, driver(cases)):
        m = Model(c['phase'], c['max_steps'], c['auto_reset'], c['light'], c['fits'])
        assert len(lines) == len(c['ks'])
        for t, (k, line) in enumerate(zip(c['ks'], lines)):
            plan, state = (list(map(int, part.split())) for part in line.split('|'))
            want_plan, phase, ready, by_task = m.step(k)
            assert plan == want_plan, (c, t, line)
            assert state[:2] == [phase, ready], (c, t, line)
            if ready:  # order_by_task means nothing without a pending order
                assert state[2] == by_task, (c, t, line)


def _case(phase, max_steps, auto_reset, light, ks, fits=1):
    return dict(phase=phase, max_steps=max_steps, auto_reset=auto_reset, light=light, fits=fits, ks=list(ks))


def test_single_steps_exhaustive(driver):
    cases = [_case(p, T, ar, li, [1] * 20)
             for T, ar, li, p in itertools.product((0, 1, 2, 3, 7), (0, 1), (0, 1), (-1, 0, 1, 2, 5))]
    assert len(cases) == 100
    _check(driver, cases)


def test_fused_call_clears_pending_order(driver):
    # k_steps 3 right after a light launch that pre-sorted (steps 1 and 5 of T = 7), and elsewhere
    cases = [_case(0, 7, 1, 1, [1, 1, 3, 1, 1, 1, 1, 1, 1]),
             _case(0, 7, 1, 1, [1, 1, 1, 1, 1, 1, 3, 1, 1, 1, 3, 1, 1]),
             _case(2, 7, 1, 1, [1, 1, 1, 1, 3, 3, 1, 1, 1]),
             _case(1, 3, 1, 1, [1, 3, 1, 1, 1]),
             _case(0, 7, 0, 1, [1, 1, 3, 1, 1, 1, 7, 1, 1]),
             _case(-1, 7, 1, 1, [1, 3, 1, 1])]
    _check(driver, cases)
    # the fused call after the pre-sort drops the order: the full step after it sorts for itself
    lines = driver([_case(0, 7, 1, 1, [1, 1, 3, 1])])[0]
    assert lines[1].split('|')[1].split()[1] == '1' and lines[2].split('|')[1].split()[1] == '0'
    assert lines[3].split()[:7] == ['0', '0', '0', '0', '1', '1', '0']


def test_more_envs_than_int32_never_orders(driver):
    cases = [_case(0, 7, 1, 1, [1] * 20, fits=0)]
    _check(driver, cases)
    for line in driver(cases)[0]:
        plan = line.split()
        assert plan[1] == '0' and plan[4] == '0' and plan[5] == '0'
