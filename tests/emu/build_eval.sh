#!/bin/bash
# tests/emu/build_eval.sh -- compile the dwgsim_eval kernels and host code against the CPU SIMT emulation shim (TEST INFRASTRUCTURE ONLY).
# Output: tests/emu/libdwgsim_eval_emu.so (the dwgsim_hip_eval_* C-ABI) and tests/emu/dwgsim_eval-emu (the command line over it).
set -e
cd "$(dirname "$0")"
SRC=../../dwgsim_amd/csrc
exec 9> .build_eval.lock; flock 9
if [ -x dwgsim_eval-emu ] && [ -f libdwgsim_eval_emu.so ] && [ -z "$(find $SRC/dw_eval.hip $SRC/dw_eval.hpp $SRC/dw_eval_launch.hpp $SRC/dw_eval.cpp $SRC/dw_mem.hpp $SRC/dwgsim_eval_cli.cpp ../../include/dwgsim_hip.h hip hip_emu.cpp build_eval.sh lds.ld check_lds.py -newer libdwgsim_eval_emu.so 2>/dev/null | head -1)" ]; then
  echo up to date: tests/emu/libdwgsim_eval_emu.so; exit 0
fi
g++ -O2 -g -std=c++17 -fPIC -shared -pthread -fdata-sections -I. -I$SRC -x c++ $SRC/dw_eval.hip $SRC/dw_eval.cpp hip_emu.cpp -Wl,-T,lds.ld -o libdwgsim_eval_emu.so.tmp
python3 check_lds.py libdwgsim_eval_emu.so.tmp $SRC/dw_eval.hip $SRC/dw_eval.hpp $SRC/dw_eval_launch.hpp
mv libdwgsim_eval_emu.so.tmp libdwgsim_eval_emu.so
g++ -O2 -g -std=c++17 -pthread $SRC/dwgsim_eval_cli.cpp -o dwgsim_eval-emu -L. -ldwgsim_eval_emu -Wl,-rpath,'$ORIGIN'
echo built tests/emu/libdwgsim_eval_emu.so tests/emu/dwgsim_eval-emu
