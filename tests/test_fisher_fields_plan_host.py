"""The host arithmetic of psfmc_fisher_rows_fields and psfmc_fisher_rows_joint (psfmc_amd/csrc/psfmc_fisher_plan.h:
fisher_fields_plan, fisher_joint_plan and the link kernel's index functions) as a stand-alone program under the host
compiler's address and undefined-behaviour sanitizers (tests/host/fisher_fields_plan_check.cpp; no GPU, nothing
loaded into python), built and run as tests/test_fisher_plan_host.py builds and runs its program."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_fisher_fields_plan_under_host_sanitizers(tmp_path):
    compiler = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert compiler, 'no host C++ compiler'
    exe = str(tmp_path / 'fisher_fields_plan_check')
    subprocess.check_call([compiler, '-std=c++17', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                           os.path.join(HERE, 'host', 'fisher_fields_plan_check.cpp'), '-o', exe])
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert done.returncode == 0 and 'fisher fields plan ok' in done.stdout, done.stdout
