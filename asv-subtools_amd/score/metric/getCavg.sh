#!/bin/bash
# Cavg of a pair-form score file, the bare number: scoreSets.sh --metric Cavg calls this as
# subtools/score/metric/getCavg.sh <trials> <score>.

[[ $# != 2 ]] && echo "usage: $0 <trials> <score>" && exit 1

subtools/computeCavg.py -pairs "$1" "$2" | awk '{print $2}'
