# dev: sourced by tools/regs.sh and tools/kernel_isa.sh -- the kernel units of raysnail_amd/csrc/Makefile and the
# source file each is compiled from.
UNITS_USAGE="common | 0 .. 8 | denoise | denoise_var | adaptive | robust | matte"
# unit_src <unit>: the unit's source file, relative to raysnail_amd/csrc
unit_src() {
    case "$1" in
        denoise | denoise_var | adaptive | robust | matte) echo "rs_$1.hip" ;;
        *) echo rs_kernels.hip ;;
    esac
}
