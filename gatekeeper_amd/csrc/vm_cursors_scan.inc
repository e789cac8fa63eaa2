            // (cursors.hpp) F_VCMP carries F_VEQ's extra word: the scan for a skipped loop's end steps over it
            else if (is_vcmp(o)) pc++;
