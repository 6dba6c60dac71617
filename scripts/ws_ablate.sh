#!/bin/bash
# Phase ablations of conv3x3_ws_kernel: builds the library with -DUNETPP_WS_DBG, runs the per-layer
# profile once per UNETPP_WS_DBG value given on the command line, then rebuilds the product library.
#   The values are sums of the bits of enum WsDbgBit in unet-_amd/csrc/ws_dbg_dev.h, the one table of them.  Results are
#   garbage -- and so are the operands of later layers: the chip's clock depends on the data, compare a layer only with
#   itself.
# usage (on the GPU box, from the repo root): [PREC=exact8] [BATCH=1] [LAYERS='conv1_3\|conv0_4'] scripts/ws_ablate.sh <value> ...
set -e
cd "$(dirname "$0")/.."
python -c 'from unet_amd import _lib; _lib.build(defines=["UNETPP_WS_DBG=1"])'
for d in "$@"; do
  echo "UNETPP_WS_DBG=$d"
  UNETPP_ALLOW_DBG_LIB=1 UNETPP_WS_DBG=$d timeout -k 10 120 python scripts/layer_profile.py ${PREC:-exact} ${BATCH:-16} 2>&1 | grep "${LAYERS:-conv0_0\|conv0_4}" || true
done
UNETPP_FORCE_BUILD=1 python __graft_entry__.py > /dev/null
