#!/bin/bash
# Device assembly of one of the setup / sensor / fix-up kernels (k_main.hip): tools/tab_asm.sh [mangled-name prefix] [extra flags]
#   -> /tmp/t/k_main.s, /tmp/t/kernel.s (+ loop summary).  The rollout kernels: tools/unit_asm.sh <unit> <prefix>.
pat=${1:-_ZN2sgL14observe_kernel}; shift
exec "$(dirname "$0")/unit_asm.sh" k_main "$pat" "$@"
