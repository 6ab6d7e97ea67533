# The resource gate of the Makefile's GATED units, on hipcc's report (-Rpass-analysis=kernel-resource-usage) of one unit:
#   awk -v unit=U -v kernel=K -v max_vgprs=N -v max_lds=N -f resource_gate.awk U.o.res        ("-": no such budget)
# Exactly one report for the kernel, no scratch, no spill, and the budgets given.  Prints the kernel's figures on one line,
# then, if the gate fails, why; the exit status is the gate's.
/Function Name:/ { k = ($NF == "[-Rpass-analysis=kernel-resource-usage]") ? $(NF-1) : $NF }
k != kernel || !/remark:/ { next }
{ v = $(NF-1) }
/Function Name|VGPRs|SGPRs|ScratchSize|Occupancy|LDS Size/ {
    s = $0; sub(/^.*remark: [^ ]* */, "", s); sub(/ \[-Rpass-analysis.*$/, "", s); gsub(/  +/, " ", s)
    line = line (line == "" ? "" : ";") s
}
/ VGPRs: /                { n++; if (max_vgprs != "-" && v + 0 > max_vgprs + 0) bad = bad " VGPRs=" v }
/ScratchSize/             { if (v + 0 != 0) bad = bad " scratch=" v }
/VGPRs Spill|SGPRs Spill/ { if (v + 0 != 0) bad = bad " spill=" v }
/LDS Size/                { if (max_lds != "-" && v + 0 > max_lds + 0) bad = bad " LDS=" v }
END {
    if (line != "") print unit ": " line
    if (n != 1 || bad != "") { print kernel " fails its resource gate:" (n != 1 ? " no resource report" : "") bad; exit 1 }
}
