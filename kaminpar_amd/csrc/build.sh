#!/bin/bash
# Builds kaminpar_amd/libkaminpar_lp.so (gfx950). Run from csrc/.
set -e
cd "$(dirname "$0")"
hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -c lp_hip.hip -o lp_hip.o
hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -c jet_hip.hip -o jet_hip.o
hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -c extract_hip.hip -o extract_hip.o
hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -c resident_hip.hip -o resident_hip.o
hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -c vcycle_hip.hip -o vcycle_hip.o
hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -c sparsify_hip.hip -o sparsify_hip.o
hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -c edges_hip.hip -o edges_hip.o
g++ -O3 -fPIC -std=c++17 -fopenmp -Wall -c graph_gen.cpp -o graph_gen.o
g++ -O3 -fPIC -std=c++17 -fopenmp -Wall -c partition_host.cpp -o partition_host.o
g++ -O3 -fPIC -std=c++17 -Wall -c pipeline_host.cpp -o pipeline_host.o
hipcc -shared -fPIC lp_hip.o jet_hip.o extract_hip.o resident_hip.o vcycle_hip.o sparsify_hip.o edges_hip.o graph_gen.o partition_host.o pipeline_host.o -o ../libkaminpar_lp.so -lgomp -L/opt/rocm/lib -lrccl
echo "built kaminpar_amd/libkaminpar_lp.so"
