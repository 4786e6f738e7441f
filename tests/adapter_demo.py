"""The little C++ programs of the adapter tests: build(tmp_path, name, source) compiles one stand-alone with g++ against
include/ and links it to liblslam_gpu.so; run(exe, *args) runs it and returns the completed process, its output captured."""
import pathlib
import subprocess

from lslam_amd import build as library

ROOT = pathlib.Path(__file__).resolve().parent.parent


def build(tmp_path, name, source):
    lib = library.build_library()
    src = tmp_path / (name + ".cpp")
    src.write_text(source)
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-I", str(ROOT / "include"), str(src), "-o", str(exe),
                    str(lib), f"-Wl,-rpath,{lib.parent}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def run(exe, *args):
    return subprocess.run([str(exe), *args], capture_output=True, text=True)
