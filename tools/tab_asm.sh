#!/bin/bash
# Device assembly of one of the setup / read-out / fix-up kernels (k_main.hip): tools/tab_asm.sh [mangled-name prefix] [extra flags]
#   -> /tmp/t/k_main.s, /tmp/t/kernel.s (+ loop summary).  The rollout kernels: tools/unit_asm.sh <unit> <prefix>; the map and
# look-ahead kernels: tools/unit_asm.sh k_obs _ZN2sgL17map_raster_kernel.
pat=${1:-_ZN2sgL21terminal_flags_kernel}; shift
exec "$(dirname "$0")/unit_asm.sh" k_main "$pat" "$@"
