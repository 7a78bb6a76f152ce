"""CPU: the labelled add_vectors overload of the host twin (quick-adc_amd/host/query_driver.hpp, driver
tests/cpp/add_labelled_host.cpp) equals the plain one with its labels mapped through the label array — the definition that
qadc_adc_index_add_vectors_labelled and qadc_index_add_vectors_labelled are held to on the GPU (tests/test_gpu_add_labelled.py)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "add_labelled_host.cpp")


def build(tmp_path, *flags):
    exe = str(tmp_path / "add_labelled_host")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Werror", *flags, SRC, "-o", exe])
    return exe


def test_the_labelled_overload_equals_the_plain_one_with_mapped_labels(tmp_path):
    out = subprocess.run([build(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


def test_the_driver_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    out = subprocess.run([build(tmp_path, "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
